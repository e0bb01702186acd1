/*
 * femshell.h -- C ABI of libfemshell, the MI355X (gfx950) implementation of
 * fem-shell's hot path: per-element flat-shell stiffness assembly and the
 * sparse solve for nodal displacements.
 *
 * This is the drop-in boundary.  Every entry point names the reference
 * interface it replaces ("SA" = src/fem-shell/fem-shell.cpp, "PC" =
 * src/fem-shell/preCICE/fem-shell_precice.cpp of precice/fem-shell).  The
 * reference-side bindings (libMesh assemble callback, LinearSolver subclass,
 * preCICE adapter loop) are shown in INTEGRATION.md.
 *
 * Conventions
 *  - plain C, host pointers, caller-owned buffers; the library copies in/out
 *  - every call returns FEMSHELL_OK (0) or a negative femshell_status; the text
 *    of the last error of the calling thread is femshell_last_error()
 *  - no exceptions cross the boundary
 *  - one context per host thread / MPI-style rank; a context is not thread-safe,
 *    distinct contexts are independent
 *  - all floating point is IEEE double (libMesh Real/Number), node ids are
 *    int32, dof of (node, var) is 6*node + var with var = u,v,w,tx,ty,tz
 *    (the layout of build_solution_vector, SA:141, 163-169)
 *  - there is NO CPU fallback: without a HIP device every compute call fails
 *    with FEMSHELL_ERR_NO_DEVICE
 */
#ifndef FEMSHELL_H
#define FEMSHELL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FEMSHELL_VERSION 2

typedef enum femshell_status {
    FEMSHELL_OK = 0,
    FEMSHELL_ERR_INVALID = -1,     /* bad argument / call order */
    FEMSHELL_ERR_NO_DEVICE = -2,   /* no usable HIP device */
    FEMSHELL_ERR_HIP = -3,         /* HIP runtime error */
    FEMSHELL_ERR_MESH = -4,        /* index out of range, degenerate element */
    FEMSHELL_ERR_BREAKDOWN = -5,   /* CG breakdown: p.Ap <= 0 (matrix not SPD) */
    FEMSHELL_ERR_COMM = -6,        /* RCCL error */
    FEMSHELL_ERR_UNSUPPORTED = -7
} femshell_status;

/* behaviour flags; FEMSHELL_REF_DEFAULT reproduces the reference as coded */
#define FEMSHELL_REF_Y21        0x1u /* SA:586: Y(2,1) = -2*x31*x31 instead of the thesis' -2*x31*y31 */
#define FEMSHELL_REF_DRILL_MAX  0x2u /* SA:1035-1052: drilling stiffness max(..)/1000 on every node block */
#define FEMSHELL_REASSEMBLE_EACH_SOLVE 0x4u /* PC:271: rebuild K on every solve (the reference does; K is constant) */
#define FEMSHELL_REF_DEFAULT    (FEMSHELL_REF_Y21 | FEMSHELL_REF_DRILL_MAX)
/* node renumbering inside the library (any number of ranks): rows are stored along a Morton curve through the mesh /
 * in reverse Cuthill-McKee order, so that the x entries a 32-node slice gathers are close together whatever the caller's
 * numbering is.  libMesh renumbers for locality by default; the reference switches it off only because its force file is
 * indexed by the original ids (SA:36).  Every node-indexed argument of this ABI keeps the caller's numbering.
 * FEMSHELL_REORDER=morton|rcm in the environment sets the flag for contexts created without one. */
#define FEMSHELL_REORDER_MORTON 0x10u
#define FEMSHELL_REORDER_RCM    0x20u

typedef struct femshell_config {
    double nu;          /* Poisson's ratio  -nu (SA:217) */
    double E;           /* Young's modulus  -e  (SA:225) */
    double thickness;   /* shell thickness  -t  (SA:233) */
    uint32_t flags;     /* FEMSHELL_REF_* | FEMSHELL_REASSEMBLE_EACH_SOLVE */
    int32_t device;     /* HIP device ordinal; -1 = the calling thread's current device */
    int32_t rank;       /* this process' index in the row partition (0 for one GPU) */
    int32_t world_size; /* number of processes = GPUs sharing the mesh (1 for one GPU) */
} femshell_config;

typedef struct femshell_ctx femshell_ctx;

/* replaces: global state nu/em/thickness/Dp/Dm + initMaterialMatrices (SA:273-294, fem-shell.h:46-52) */
int femshell_create(const femshell_config *cfg, femshell_ctx **out);
int femshell_destroy(femshell_ctx *ctx);
const char *femshell_last_error(void);

/* replaces: what assemble_elasticity reads through es.get_mesh()/DofMap (SA:1166-1205):
 * the replicated mesh (SA:35-37).  xyz[n_nodes][3]; tri[n_tri][3]; quad[n_quad][4]
 * (either count may be 0).  Every rank passes the same global mesh; the library keeps
 * the node rows [femshell_row_begin, femshell_row_end) of its rank plus the ghost
 * nodes/elements they touch, and builds the block sparsity (libMesh does this in
 * EquationSystems::init, SA:125).  FEMSHELL_ERR_MESH: an invalid mesh (index out of range,
 * repeated node, unattached node).  FEMSHELL_ERR_UNSUPPORTED: a valid mesh beyond a limit of
 * the layout (more than 765 elements at a node, more than 4095 elements or too many for the
 * assembly kernel's LDS on one 32-node slice, more than 63 neighbours of a node in full
 * storage); the context stays usable, but has no mesh until one is accepted: nothing of the
 * previous mesh (K, the solution, the multigrid hierarchy) is valid any more. */
int femshell_set_mesh(femshell_ctx *ctx, int32_t n_nodes, const double *xyz, int32_t n_tri,
                      const int32_t *tri, int32_t n_quad, const int32_t *quad);

typedef struct femshell_section { double nu, E, thickness; } femshell_section;
/* extends: the global nu / em / thickness of the reference (SA:217-233, initMaterialMatrices SA:273-294) to one
 * set per element ("shell sections": flanges thicker than the web, a doubler on a skin, an insert of another metal, a
 * tapered thickness).  sections[n_sections]; tri_section[n_tri] / quad_section[n_quad]: index into `sections` for
 * every element of the mesh last passed to femshell_set_mesh, in the caller's element order (NULL allowed only
 * where that count is 0).  Every rank passes the same full arrays (as for femshell_set_mesh).  n_sections == 0
 * returns the context to the uniform material of its femshell_config.  Only values change: the plan and the
 * sparsity are kept, K and the multigrid hierarchy are rebuilt at the next assemble / solve.  femshell_set_mesh
 * forgets the sections (the element count may have changed).  The behaviour flags stay the context's.
 * Every call -- also one that clears, or clears when none were set -- forgets the densities of femshell_set_density and the
 * expansion coefficients of femshell_set_expansion, which belong to the sections they were given for, and with alpha the
 * temperatures of femshell_set_thermal: the loads in force go back to nodal + S and the right-hand side is rebuilt.
 * FEMSHELL_ERR_INVALID (no mesh, a null array, an index outside [0, n_sections), a section that femshell_create
 * would refuse as a config) leaves the sections that were in force untouched.
 * A context with sections runs the sectioned instantiation of the kernel its mesh was laid out for; the pipelined one takes
 * slices of at most 134 triangles then (longer records), and a mesh between that and the uniform limit of 150 is assembled by
 * the two-phase kernel while it has sections.  femshell_assembly_kernel reports what a context will in fact launch. */
int femshell_set_sections(femshell_ctx *ctx, int32_t n_sections, const femshell_section *sections,
                          const int32_t *tri_section, const int32_t *quad_section);

/* replaces: DirichletBoundary {0,20}->u,v,w and {1,21}->all six (SA:90-120).  mask6 bit v
 * fixes dof v of the node to 0.  node_ids == NULL: mask6 has one byte per node (n == n_nodes).
 * Calling it again replaces the previous set. */
int femshell_set_dirichlet(femshell_ctx *ctx, int32_t n, const int32_t *node_ids, const uint8_t *mask6);

/* extends: the homogeneous DirichletBoundary of the reference (SA:90-120, every fixed dof is fixed to 0) to NON-ZERO prescribed
 * displacements: support settlement, displacement-controlled loading, a sub-model driven by a coarse model's displacements.
 * u6[n][6]; the argument forms of femshell_set_loads: node_ids == NULL needs n == n_nodes, nodes not listed get 0, n == 0 clears;
 * a non-finite value returns FEMSHELL_ERR_INVALID and leaves the values that were in force untouched.  Only the entries at dofs
 * the Dirichlet set fixes are used -- entries at free dofs are IGNORED --, and that is decided when the right-hand side is built:
 * the order of femshell_set_dirichlet and femshell_set_prescribed does not matter.  femshell_set_mesh forgets the values.
 *
 * With u = u_h + u_bar (u_bar: the prescribed values at the fixed dofs, 0 elsewhere) the system solved is the one of the
 * homogeneous set with the right-hand side
 *     F = mask(loads - K_unc u_bar),
 * K_unc the stiffness WITHOUT constraints.  K_unc is never stored (the assembly writes zero rows and columns with a counting
 * diagonal at fixed dofs): the product is formed on the device from the element matrices (csrc/element_product.hip), one launch
 * per right-hand side.  Only the right-hand side is rebuilt: K, block-Jacobi and the multigrid hierarchy are kept.  With no fixed
 * dof carrying a non-zero value the right-hand side is built exactly as without this call.
 * The solvers and the solution vector in HBM see the homogeneous part u_h (zero on fixed dofs; femshell_set_initial_guess(NULL)
 * starts from it, an explicit u0 counts on the free dofs only); u_bar is put in where a solution leaves the library:
 * femshell_get_solution and u_out of femshell_solve return u, with the prescribed values at the fixed dofs bit for bit.
 * femshell_export_bsr's F and femshell_residual see the F above.  femshell_modes is unaffected (it solves on the free dofs).
 * FEMSHELL_ERR_INVALID while dynamics is active (and femshell_dynamics_begin returns it while prescribed values are in force, i.e.
 * until n == 0 clears them: a Newmark step with moving supports is an open end).  FEMSHELL_ERR_UNSUPPORTED on a row-partitioned
 * context (world_size != 1): the ghost values of u_bar and a halo exchange in front of the element product are an open end. */
int femshell_set_prescribed(femshell_ctx *ctx, int32_t n, const int32_t *node_ids, const double *u6);

/* replaces: the global `forces` vector read by contribRHS (SA:44-67, 1118-1153; PC:1377-1438).
 * f6[n][6] nodal forces and moments; node_ids == NULL: one row per node (n == n_nodes).
 * Nodes not listed get zero load.  Only the right-hand side is rebuilt. */
int femshell_set_loads(femshell_ctx *ctx, int32_t n, const int32_t *node_ids, const double *f6);

/* extends: the reference knows nodal forces only (its `_f` file; its mesh generator lumps a pressure to nodes by an h^2 rule)
 * to DISTRIBUTED loads per element: pressure on the surface, weight or snow per area.  Per element four doubles (p, qx, qy, qz):
 *   p   pressure, force per area, along the element's own +ez: the normal K is built with and the "top surface" of
 *       femshell_element_resultants.  TRI3: ez || (b-a) x (c-a); QUAD4: ez || d1 x d2 with the diagonals d1 = c-a, d2 = d-b
 *       (the direction of the element frame's ez: (mid1-mid3) x (mid2-mid0) = d1 x d2 / 2).  The load is DEAD: it follows the
 *       undeformed geometry, it is not a follower load.
 *   q   traction, force per area of the element's true area, in global axes (self-weight rho t g, snow).
 * The nodal equivalents are LUMPED, with the shares of femshell_lumped_mass:
 *     TRI3   every node gets  p (b-a) x (c-a) / 6 + q A / 3,   A = |(b-a) x (c-a)| / 2
 *     QUAD4  every node gets  p (d1 x d2) / 8     + q A / 4,   A = |d1 x d2| / 2
 * on u, v, w; the rotational rows receive nothing.  The pressure part is the exact resultant of p on the element (the vector area
 * of a skew quadrilateral is d1 x d2 / 2); the traction part with q = rho t g is g times the element's translational lumped
 * mass.  This is the work-equivalent load of the linear / bilinear membrane interpolation: the consistent nodal MOMENTS of
 * Specht's and the DKQ bending fields are left out on purpose.  The deflection converges with h^2.
 * S_a = the sum over the elements that contain node a, taken in the order of the element list of the node's slice, starting from
 * zero, without atomics: bitwise reproducible, independent of grid and tile size.  The loads in force are
 *     loads_a = nodal_a + S_a   (one rounding),
 * nodal the loads of femshell_set_loads: F, the right-hand side with prescribed values, femshell_reactions (K_unc u - (nodal + S):
 * its force columns balance the total load) and the Newmark right-hand side all see the sum.  A degenerate element contributes
 * what the formula gives: a zero vector area, no status.
 * tri_load[n_tri][4] / quad_load[n_quad][4]: rows in the caller's element order; every rank passes the full arrays (as for
 * femshell_set_sections).  NULL for one kind leaves that kind unloaded; both NULL clears the element loads.  The call replaces the
 * previous set; only the right-hand side is rebuilt, and the nodal loads are not uploaded again (32 bytes per local element are).
 * Allowed wherever femshell_set_loads is: while dynamics is active (F of the next step), with prescribed values in force, on
 * row-partitioned contexts.  FEMSHELL_ERR_INVALID (a non-finite value, no mesh) leaves what was in force untouched.
 * femshell_set_mesh forgets the element loads; femshell_set_sections and femshell_set_density do not touch them (the values are
 * the caller's per-area numbers).  Kernel: csrc/element_loads.hip. */
int femshell_set_element_loads(femshell_ctx *ctx, const double *tri_load /* n_tri x 4, or NULL */,
                               const double *quad_load /* n_quad x 4, or NULL */);
/* f6_out[n_nodes][6]: S alone, the nodal equivalents of the element loads in force, in the caller's numbering, NOT masked by the
 * Dirichlet set; on a row-partitioned context every rank receives all rows (gathered like femshell_lumped_mass).  Zeros when no
 * element loads are set.  Two calls give the same bits. */
int femshell_element_load_vector(femshell_ctx *ctx, double *f6_out /* n_nodes x 6 */);

/* extends: the reference has no thermal loads.  TEMPERATURE per element: two doubles (Tm, Tg),
 *   Tm  the temperature change of the mid-surface,
 *   Tg  = T_top - T_bottom, the difference through the thickness; "top" is z = +t/2 along the element's own ez, the top of
 *       femshell_element_resultants and the normal the pressure of femshell_set_element_loads acts along,
 * and per context an expansion coefficient alpha, optionally one per section (passed as femshell_set_density passes rho:
 * n_sections == 0: alpha for every element; otherwise n_sections must be the context's section count).
 * Free thermal state in the element frame, kappa = (w,xx, w,yy, 2 w,xy) as in the resultants:
 *     eps0 = alpha Tm (1, 1, 0),   kappa0 = -(alpha Tg / t) (1, 1, 0)
 * (a plate that is warmer on top bows towards +ez in the middle of its edges' chord: w,xx < 0).  Stress state, exact for a
 * temperature that is linear through the thickness:
 *     N_loc = t Dm (eps - eps0),   M_loc = -Dp (kappa - kappa0).
 * Equivalent nodal loads, work-equivalent, with the element's OWN strain operators and the quadrature of its stiffness:
 *     f_m = sum_g w_g Bm_g^T (t Dm eps0) =  N_T sum_g w_g Bm_g^T (1,1,0),   N_T = E t alpha Tm / (1 - nu)
 *     f_p = sum_g w_g Bp_g^T (Dp kappa0) = -M_T sum_g w_g Bp_g^T (1,1,0),   M_T = E t^2 alpha Tg / (12 (1 - nu))
 * TRI3: the CST operator at one point (f_m of a node is N_T / 2 times the in-plane normal of the opposite side that points towards
 * the node -- outward at the node: a heated element pushes its nodes apart --, scaled by the side's length) and Specht's curvature operator at its three Gauss points, with the Y of the stiffness (FEMSHELL_REF_Y21
 * included; the row of Y that the switch changes multiplies the zero of (1,1,0)).  QUAD4: the bilinear membrane operator and MINUS
 * the DKQ operator at the 2 x 2 points with weights det J.  The loads are rotated to global axes with the element frame; they fill
 * the rotational rows, the drilling row gets nothing.  A degenerate element contributes finite zeros and reports no status here
 * (the assembly reports it).
 * T_a = the sum over the elements that contain node a, in the order of the element list of the node's slice, from zero, without
 * atomics: bitwise reproducible, independent of grid and tile size.  The loads in force are
 *     loads_a = (nodal_a + S_a) + T_a   (one rounding per +),
 * S the element loads: F, the right-hand side with prescribed values, femshell_reactions (r = K_unc u - loads: the internal force
 * is K u - T) and the Newmark right-hand side all see the sum.  With no temperatures set every buffer and every bit is what it is
 * without these functions.  While temperatures are in force femshell_element_resultants reports the stress state above (and the
 * surface stresses computed from it), and femshell_geometric_product / femshell_buckling use its membrane forces.
 * tri_temp[n_tri][2] / quad_temp[n_quad][2]: rows in the caller's element order; every rank passes the full arrays.  NULL for one
 * kind leaves that kind cold; both NULL clears the temperatures.  The call replaces the previous set; only the right-hand side is
 * rebuilt, and the nodal loads are not uploaded again (16 bytes per local element are).  Allowed wherever
 * femshell_set_element_loads is.  FEMSHELL_ERR_INVALID (a non-finite value, no mesh, temperatures before alpha is set, a section
 * count that does not match) leaves what was in force untouched.  femshell_set_expansion while temperatures are in force rebuilds
 * the loads with the new alpha.  femshell_set_mesh forgets the temperatures and alpha; femshell_set_sections forgets alpha -- as
 * it forgets the densities -- and with it the temperatures: the loads are nodal + S again.  Kernel: csrc/element_thermal.hip. */
int femshell_set_expansion(femshell_ctx *ctx, double alpha, int32_t n_sections, const double *section_alpha);
int femshell_set_thermal(femshell_ctx *ctx, const double *tri_temp /* n_tri x 2, or NULL */,
                         const double *quad_temp /* n_quad x 2, or NULL */);
/* f6_out[n_nodes][6]: T alone, in the caller's numbering (also under FEMSHELL_REORDER), NOT masked by the Dirichlet set; on a
 * row-partitioned context every rank receives all rows (gathered like femshell_element_load_vector).  Zeros when no temperatures
 * are set.  Two calls give the same bits. */
int femshell_thermal_load_vector(femshell_ctx *ctx, double *f6_out /* n_nodes x 6 */);

/* extends: every support the reference knows is rigid (a dof is fixed or free).  ELASTIC SUPPORTS: a plate on soil (a Winkler
 * foundation), a panel on elastomer pads, a bolt or a neighbouring structure as a spring at a node, a free-floating shell made
 * solvable without inventing Dirichlet nodes.
 *
 * Foundation, per element.  Each element gets two doubles (kn, kt), both >= 0, in force per volume (pressure per unit
 * deflection).
 *   kn acts along the element's own +ez.  This is the normal of femshell_set_element_loads: TRI3 c = (b-a) x (c-a), QUAD4
 *      c = d1 x d2.
 *   kt acts in the element's plane.
 * The foundation is lumped with the shares of femshell_lumped_mass.  Every node of element e gets the 3 x 3 block
 *     B_e = share_e [ kt I + (kn - kt) n n^T ],   share_e = A_e/3 (TRI3), A_e/4 (QUAD4),
 *     A_e = |c|/2,   n = c/|c|
 * A degenerate element (|c| = 0) contributes zero and reports nothing, as in the element loads.  The rotational rows get nothing.
 * T_a = sum over the elements e that contain node a of B_e is taken in the order of the slice's element list, from zero.  It is
 * stored as six words xx, yy, zz, xy, yz, zx, the project's tensor order.
 *
 * Springs, per node.  Each node gets six doubles (kx, ky, kz, krx, kry, krz), all >= 0, in global axes.
 *
 * Support table.  Per node nine doubles:
 *   words 0-5: T_a with kx, ky, kz added to its three diagonal words (one addition each, after the row sum);
 *   words 6-8: krx, kry, krz.
 * K_sup is the block-diagonal matrix of these.
 *
 * The matrix in HBM.  After every assembly, K in HBM is K + mask(K_sup).  Entry (i, j) of a node's diagonal block receives one
 * addition, fl(K_ij + S_ij), where neither dof i nor dof j of that node is fixed.  Nothing is added at fixed dofs, which keep the
 * assembly's identity rows.  All other blocks are untouched, bit for bit.
 *
 * What follows from it: femshell_solve solves the supported shell, with either preconditioner; femshell_spmv / spmm / residual /
 * export_bsr give products and blocks of K + mask(K_sup); dynamics steps with K + K_sup + c M; femshell_modes and
 * femshell_buckling see the supported shell; with non-zero prescribed values F = mask(loads - K_unc u_bar - K_sup u_bar);
 * femshell_reactions gives r = K_unc u + K_sup u - loads -- the negative residual at free dofs, the rigid support's reaction at
 * fixed ones: over all nodes the force columns of r + femshell_support_forces + loads sum to zero.  femshell_element_product,
 * femshell_element_matrices, femshell_geometric_product, femshell_element_resultants and femshell_nodal_resultants are the
 * shell's own: supports carry no shell stress.
 *
 * femshell_set_foundation: tri_k[n_tri][2] / quad_k[n_quad][2], rows (kn, kt) in the caller's element order; every rank passes
 * the full arrays.  NULL for one kind leaves that kind without a foundation; both NULL clears the foundation.  The call replaces
 * the previous set.
 * femshell_set_springs: the conventions of femshell_set_loads (node_ids == NULL: one row per node, n == n_nodes); unlisted nodes
 * get no spring; n == 0 clears the springs.  The call replaces the previous set.
 * Both work on row-partitioned contexts.  A changed or cleared set makes K, F, block-Jacobi and the multigrid hierarchy stale:
 * the next use assembles again (nothing is subtracted in place).  FEMSHELL_ERR_INVALID: a negative or non-finite value, no mesh,
 * an id out of range or listed twice, a call while dynamics is active (K_eff lies in HBM).  Every refusal leaves what was in
 * force untouched and the context usable.  femshell_set_mesh forgets both sets; femshell_set_sections, femshell_set_dirichlet
 * and femshell_set_density keep them (the moduli are the caller's numbers, and the mask is applied at the next assembly).  With
 * nothing set every buffer, every launch and every bit is what it is without these functions.
 * Kernels: csrc/elastic_support.hip. */
int femshell_set_foundation(femshell_ctx *ctx, const double *tri_k /* n_tri x 2, or NULL */, const double *quad_k /* n_quad x 2, or NULL */);
int femshell_set_springs(femshell_ctx *ctx, int32_t n, const int32_t *node_ids, const double *k6);
/* out[n_nodes][9]: the support table in force, in the caller's numbering, NOT masked by the Dirichlet set; on a row-partitioned
 * context every rank receives all rows (gathered like femshell_lumped_mass).  Zeros when nothing is set.  Two calls give the
 * same bits, at every grid size. */
int femshell_support_stiffness(femshell_ctx *ctx, double *out /* n_nodes x 9 */);
/* f6_out[n_nodes][6] = -K_sup u, the force and moment the elastic supports exert on the shell, in the caller's numbering; u ==
 * NULL: the last solution (with the prescribed values in force added).  Needs a mesh, not an assembled K.  Zeros when nothing is
 * set.  FEMSHELL_ERR_UNSUPPORTED on a row-partitioned context, like femshell_reactions. */
int femshell_support_forces(femshell_ctx *ctx, const double *u /* n_nodes x 6, or NULL */, double *f6_out /* n_nodes x 6 */);

/* replaces: assemble_elasticity (SA:1160-1233): element stiffness (initElement, calcPlane,
 * calcPlate, constructStiffnessMatrix, localToGlobalTrafo), constraint handling, add_matrix /
 * add_vector.  K and F stay in HBM. */
int femshell_assemble(femshell_ctx *ctx);
/* The same assembly without the round trip that collects its status: the kernels are enqueued and the call returns.  A
 * degenerate element (FEMSHELL_ERR_MESH) -- on any rank of the row partition -- is reported by the next call on this context
 * that synchronises, reads K or changes its inputs: femshell_sync, femshell_solve, femshell_assemble, femshell_export_bsr,
 * femshell_spmv, femshell_residual, femshell_set_dirichlet, femshell_set_loads.  For callers that assemble in a loop
 * (re-meshing, time stepping with changing geometry): on 8 ranks the agreement on the status costs as much as the 0.08 ms
 * assembly step itself.  Multi-rank contexts: every rank makes the same sequence of calls, as for femshell_assemble. */
int femshell_assemble_async(femshell_ctx *ctx);

typedef struct femshell_solve_info {
    int32_t iterations;     /* CG iterations performed */
    int32_t converged;      /* 1: ||r|| <= rtol*||b|| (multigrid with refinement: <= 100 rtol*||b|| after the first phase,
                               then the refinement pass -- see femshell_pc_options::refine_passes), 0: max_it reached */
    double rel_residual;    /* recurrence ||r||_2 / ||b||_2 at exit (what the stopping rule tests; multigrid with
                               refinement: at the end of the first phase) */
    double true_rel_residual; /* ||b - K u||_2 / ||b||_2 recomputed explicitly after a converged solve, -1 if not
                               computed (rtol <= 0, iteration limit, breakdown).  On ill-conditioned shells the
                               recurrence drifts and this floors near kappa*eps; it is reported, not enforced:
                               restarting CG from the explicit residual was tried and made the error worse */
    double assemble_seconds;/* device time of the assembly done inside this call (0 if reused) */
    double setup_seconds;   /* block-Jacobi factorisation */
    double solve_seconds;   /* CG loop, device time */
    double bytes_per_iteration; /* algorithmic HBM bytes of one CG iteration on this rank */
    int32_t pc_type;        /* femshell_pc_type the solve ran with */
    int32_t amg_levels;     /* levels of the multigrid hierarchy (0 with block-Jacobi) */
    double pc_setup_seconds;/* host + device time of the multigrid setup done inside this call (0 if reused) */
    double operator_complexity; /* sum of the level matrices' blocks / blocks of K (0 with block-Jacobi) */
    /* error estimate of the multigrid-preconditioned solve (version 2 of this struct; -1 / 0 when no refinement pass ran):
     * a refinement pass solves K e = b - K x (residual in double-double) and adds e, so ||e||/||x|| of the last pass
     * measures the relative displacement error of the iterate BEFORE that pass, and the pass leaves behind about
     * that times the factor by which it reduced the residual of its correction equation.  Checked against manufactured
     * solutions at the 4M-triangle sizes (tests/test_gpu_fullsize.py, bench.py time_to_solution.manufactured). */
    int32_t refine_passes_done;       /* refinement passes that ran (<= femshell_pc_options::refine_passes + 1) */
    int32_t pc_fp64_fallback;         /* 1: the flexible CG broke down (p.Ap <= 0) under a multigrid hierarchy that keeps
                                         single-precision copies, and the solve ran again from the start with an all-FP64
                                         hierarchy (very thin shells); the context keeps that choice until a new mesh or
                                         preconditioner is set.  (the reserved word of version 2 of this struct) */
    double refine_correction_rel;     /* ||e||_2 / ||x||_2 of the last pass */
    double refine_residual_reduction; /* ||rhs - K e|| / ||rhs|| (recurrence) the last pass stopped at */
    double error_estimate;            /* refine_correction_rel * refine_residual_reduction: estimated relative error of u */
} femshell_solve_info;

/* ---- preconditioner ------------------------------------------------------------------
 * replaces: the -ksp_type / -pc_type options the reference passes through to PETSc
 * (doc/implementation.tex:68-72; equation_systems.parameters stay untouched, SA:130-133).
 * The Krylov method is always CG (K is SPD).  FEMSHELL_PC_BLOCK_JACOBI (default) is the 6x6
 * point-block Jacobi whose iterates the CPU oracle reproduces step by step; its iteration
 * count grows with the element count.  FEMSHELL_PC_AMG is a smoothed-aggregation multigrid
 * (rigid-body modes, Chebyshev/block-Jacobi smoothing, V or K cycle) around which the solve
 * runs a flexible CG: the answer a user of `-pc_type gamg` expects, with iteration counts
 * that stay near 100 up to the 4M-triangle meshes.  On row-partitioned contexts the hierarchy is
 * row-partitioned like K (aggregates never span ranks; levels above 60,000 nodes split over the
 * ranks, the rest replicated): iteration counts within a few of the single-rank ones.  What the
 * cycle only smooths or transfers with is kept in single precision (FP64 arithmetic); should the
 * flexible CG break down under it, the solve runs again with an all-FP64 hierarchy
 * (femshell_solve_info::pc_fp64_fallback).
 * The environment variable FEMSHELL_PC=amg|jacobi sets the default of new contexts. */
typedef enum femshell_pc_type { FEMSHELL_PC_BLOCK_JACOBI = 0, FEMSHELL_PC_AMG = 1 } femshell_pc_type;
typedef enum femshell_cycle { FEMSHELL_CYCLE_V = 0, FEMSHELL_CYCLE_K = 1 } femshell_cycle;
typedef struct femshell_pc_options {
    int32_t type;            /* femshell_pc_type */
    int32_t cycle;           /* femshell_cycle (default K: two flexible-CG steps per coarse level) */
    int32_t smoother_degree; /* Chebyshev degree on the finest level (default 3) */
    int32_t coarse_degree;   /* Chebyshev degree on the coarser levels (default 4) */
    int32_t coarsest_nodes;  /* coarsening stops at the first level of at most this many nodes; dense inverse there (default
                                and maximum 1400: the K cycle visits its last levels 8-16 times per iteration and each
                                visit is a chain of launches, so an exact solve of 8400 dofs -- one dense matrix-vector
                                product -- is cheaper than two more levels; inverses beyond 64 nodes are computed on the
                                matrix cores) */
    int32_t max_levels;      /* default 12 */
    int32_t refine_passes;   /* iterative refinement after convergence, at most this many passes (default 1; 0 = off):
                                the residual of the iterate is evaluated in double-double and the correction equation
                                solved by the same method -- rtol bounds the residual, and on these systems the
                                displacement error sits one to two decades above it (4M triangles, manufactured
                                solution: 4e-9 at a residual of 9e-11 ||b||) -- until femshell_solve_info::error_estimate
                                of the pass so far, ||e|| / ||x|| x the drop of its residual, is a fifth of rtol (a drop
                                between 1e-2 and 1e-6; 1e-4 flat before round 5 and with FEMSHELL_REFINE_ADAPTIVE=0).  The
                                first pass always runs, further ones (one more than this number at most) while
                                femshell_solve_info::error_estimate exceeds rtol.  Plain FP64 CG stalls at a displacement
                                error of kappa*eps -- 2e-10 on the 250k-triangle roof -- one pass brings it to 1e-13.
                                With refinement on, the recurrence of the first phase runs to 100 rtol only: what rtol
                                is for is the displacement error, the pass reduces the error of whatever iterate it
                                starts from by its drop, and the digits between 100 rtol and rtol are the ones the
                                recurrence's rounding noise spoils (4M triangles: 132 instead of 148 iterations, error
                                estimate 4e-12; manufactured solutions 1e-12 / 2e-11) */
    int32_t reserved;
    double eig_ratio;        /* the smoother targets [lambda_max/eig_ratio, lambda_max] of D^-1 A (default 30) */
} femshell_pc_options;
/* fills *out with the defaults of `type` */
int femshell_pc_defaults(int32_t type, femshell_pc_options *out);
/* takes effect at the next femshell_solve; the hierarchy is rebuilt whenever K changes */
int femshell_set_preconditioner(femshell_ctx *ctx, const femshell_pc_options *opt);

/* inspection of the multigrid hierarchy of the last solve (tests; host copies are kept for
 * matrices of up to 2M blocks): level 0 is K itself.  There is none from the moment K is stale
 * (a new mesh, Dirichlet set or sections, an assembly, the start or end of dynamics) until the
 * next solve builds one. */
typedef struct femshell_amg_level_info {
    int32_t n_nodes;        /* block rows of the level */
    int32_t n_coarse;       /* aggregates = block rows of the next level (0 on the coarsest) */
    int64_t nnz_blocks;     /* blocks of the level matrix */
    int64_t p_blocks;       /* blocks of the prolongator to this level from the next (0 on the coarsest) */
    double lambda_max;      /* upper end of the smoother's interval for D^-1 A */
} femshell_amg_level_info;
int32_t femshell_amg_levels(femshell_ctx *ctx);
int femshell_amg_level(femshell_ctx *ctx, int32_t level, femshell_amg_level_info *info);
enum { FEMSHELL_AMG_AGGREGATES = 0, /* int32 [n_nodes] */
       FEMSHELL_AMG_A_ROWPTR, FEMSHELL_AMG_A_COLS, FEMSHELL_AMG_A_VALS,   /* int64 [n+1], int32 [nnzb], double [nnzb*36] */
       FEMSHELL_AMG_P_ROWPTR, FEMSHELL_AMG_P_COLS, FEMSHELL_AMG_P_VALS,
       /* the coarsest level only: the dense inverse the cycle multiplies with, double [n][n] row-major (n = 6 x its nodes;
        * the operator it inverts is that level's FEMSHELL_AMG_A_*, kept at every problem size) */
       FEMSHELL_AMG_COARSE_INVERSE,
       /* level 0: the cluster of rigidly coupled nodes every node belongs to, or -1 (the patch smoother of shells of poor element
        * quality, csrc/amg_patch.hpp); -1 as a count: the level has no clusters.  int32 [n_nodes], internal numbering */
       FEMSHELL_AMG_PATCH_LABELS };
/* returns the element count of the array (-1: not available); copies it to out when out != NULL.  The host copies behind
 * the A_* / P_* / AGGREGATES arrays are kept for problems of up to 300,000 blocks of K (up to 2,000,000 with
 * FEMSHELL_AMG_KEEP_HOST=1 in the environment at setup): an inspection interface, not part of the solve */
int64_t femshell_amg_export(femshell_ctx *ctx, int32_t level, int32_t which, void *out);
/* z = M^-1 r: ONE application of the multigrid preconditioner (the V or K cycle femshell_solve applies once per iteration, from
 * the unfused start of its level-0 smoothing), on the hierarchy of the current K -- built first, as femshell_solve builds it,
 * when the context has none.  A test entry: it holds the cycle to a restatement evaluated on the exported hierarchy.  r, z: 6
 * values per node, the caller's numbering (single rank: all nodes); on a row-partitioned context the call is collective and
 * every rank passes and receives its owned rows in the order of femshell_owned_nodes.  A later solve is not affected.
 * FEMSHELL_ERR_UNSUPPORTED with the block-Jacobi preconditioner. */
int femshell_pc_apply(femshell_ctx *ctx, const double *r, double *z);
/* the patch smoother of level 0 of the last setup (csrc/amg_patch.hpp; FEMSHELL_AMG_PATCH_TAU / _MAX in the environment): out[0] =
 * rigid edges found (sigma_max of the scaled coupling above tau), out[1] = clusters, out[2] = nodes in clusters, out[3] = clusters
 * whose diagonal block was not positive definite (they keep their point blocks), out[4] = tau, out[5] = nodes per cluster at most.
 * All zero on a mesh without such edges: nothing of the method runs then. */
int femshell_amg_patch_info(femshell_ctx *ctx, double out[6]);
/* device timings of the first coarsening step of the last setup: out[0..3] = milliseconds of the prolongator, A P,
 * restriction and Galerkin kernels, out[4] = useful flops of the Galerkin product, out[5] = flops issued on the
 * matrix cores (v_mfma_f64_16x16x4_f64 tiles; 0 when the vector-ALU kernel ran), out[6] = 1 if the matrix cores ran */
int femshell_amg_setup_stats(femshell_ctx *ctx, double out[7]);
/* Where the integer work of the last multigrid setup's coarsening steps ran (the setup is part of what replaces
 * equation_systems.solve(), fem-shell.cpp:138 -- PETSc's KSPSetUp): out[0] = steps whose patterns were built in HBM
 * (csrc/amg_symbolic.hip), out[1] = steps that took the host's lists although the device was asked (a row beyond the lane sets),
 * out[2] = steps on the host's lists by rule (clusters of rigidly coupled nodes, FEMSHELL_AMG_SYMBOLIC=host). */
int femshell_amg_symbolic_info(femshell_ctx *ctx, int32_t out[3]);
/* the dense inverse of the coarsest operator when it was computed on the matrix cores (csrc/amg_dense.hip; symmetric block
 * sweeps on v_mfma_f64_16x16x4_f64): out[0] = dofs n (0: the host inverted a small operator), out[1] = milliseconds,
 * out[2] = flops issued on the matrix cores, out[3] = n^3 (the flops of a symmetric inversion), out[4] = dropped
 * (semi-definite) directions, out[5] = bytes of the lower triangle read and written over all steps */
int femshell_amg_dense_stats(femshell_ctx *ctx, double out[6]);
/* For tests: the device dense inverse (csrc/amg_dense.hip) of a caller's SPD block CSR matrix (6 x 6 blocks, row-major; the
 * arguments and their validation are those of femshell_amg_host_dense_inverse, femshell_plan.h), on the context's streams and
 * with the setup's run-again-without-look-ahead path.  inv_out: (6 n_nodes)^2 doubles (single_precision != 0: the stored floats,
 * widened); stats_out (may be NULL): the six numbers of femshell_amg_dense_stats for this call.  The context's own hierarchy and
 * state are not touched.  FEMSHELL_ERR_BREAKDOWN where the multigrid setup would return it. */
int femshell_amg_device_dense_inverse(femshell_ctx *ctx, int32_t n_nodes, const int32_t *rowptr, const int32_t *colidx,
                                      const double *vals, int32_t single_precision, double *inv_out, double stats_out[6]);
/* For tests: one product y = inv b by the kernel every multigrid cycle applies the dense inverse with (k_dense_gemv_big), no gate.
 * inv: n x n doubles, stored on the device with the production leading dimension (as_float != 0: rounded to float first);
 * b: n doubles (uploaded zero-padded); y: n_pad6 + 8 doubles, uploaded as they are and copied back after the launch -- the
 * kernel writes rows [0, n_pad6), zeros in [n, n_pad6). */
int femshell_amg_dense_apply(femshell_ctx *ctx, int32_t n, int32_t n_pad6, const double *inv, int32_t as_float, const double *b,
                             double *y);
/* For tests: the block-Jacobi setup kernel (k_block_jacobi) on a caller's block CSR matrix (arguments and validation as above),
 * packed and uploaded as a coarse level operator of the multigrid is -- symmetric_storage 0: every block; 1: diagonal and upper
 * blocks with their in-lists; 2: as 1 and read as K itself is under symmetric storage, the strict lower triangle of a diagonal
 * block taken from its mirror image and never loaded -- with a status word of this call.  inv_out: n_nodes x 36, the inverse
 * diagonal blocks unpacked from the 21 stored words to full symmetric blocks; *status_out: 0, or -(a + 1) of a node a whose
 * diagonal block is not positive definite (its inverse is then the identity).  The context's matrix, hierarchy and state are
 * not touched. */
int femshell_amg_device_block_jacobi(femshell_ctx *ctx, int32_t n_nodes, const int32_t *rowptr, const int32_t *colidx,
                                     const double *vals, int32_t symmetric_storage, double *inv_out, int32_t *status_out);
/* For tests: the block-Jacobi inverse the context holds, n x 36 doubles as full symmetric blocks.  level 0: of K (block-Jacobi
 * and multigrid contexts; n = nodes of the mesh, in the caller's numbering); level >= 1: of that level operator of the multigrid
 * hierarchy (n = its nodes).  single_precision != 0: the copy the smoothers read, widened; FEMSHELL_ERR_INVALID where the level
 * keeps none, and for a level the context does not have.  Assembles and builds what is missing, as femshell_pc_apply does.
 * One rank only: FEMSHELL_ERR_UNSUPPORTED for a row-partitioned context. */
int femshell_block_jacobi_export(femshell_ctx *ctx, int32_t level, int32_t single_precision, double *out);
/* For tests: z = D^-1 r with that inverse by one of its two readers -- path 0: one lane per row through LDS (the kernel of the
 * power iteration, arithmetic of the CG kernels); path 1: one lane per node (the first Chebyshev step with 1 / theta = 1 on the
 * level as the smoothers see it: the single-precision copy where the level has one).  r and z: 6 x 32 x ceil(n / 32) doubles,
 * the level's padded vector as it lies in HBM (level 0 of a renumbering context: the library's numbering).  Same refusals. */
int femshell_block_jacobi_apply(femshell_ctx *ctx, int32_t level, int32_t path, const double *r, double *z);
/* ---- For tests: the Krylov loops launch by launch (csrc/api_krylov_probe.cpp).  "Set, launch one, get" on the
 * context's own CG state -- the vectors and scalars femshell_solve iterates in -- through the production launchers and nothing
 * else.  No production path runs through these.  All three refuse (FEMSHELL_ERR_INVALID, the context as it was) without a mesh,
 * without an assembled K and its block-Jacobi inverse, and while dynamics is active; they never assemble or build anything. */
/* A plain mirror of the scalars of the recurrence in HBM (csrc/kernels.hpp CgScalars: same size, same offsets). */
typedef struct femshell_krylov_scalars {
    double rz, alpha, beta, rr, bb, tol2;
    double red[3];
    int32_t done, iters;
    uint32_t ticket, pad;
    double stage[3][64];
    double ring_rz[2], ring_alpha[2];
    double pass_xx, pass_rhs_rr, pass_rtol;
} femshell_krylov_scalars;
enum {
    /* node vectors, n_nodes x 6 in the caller's numbering (a row-partitioned context moves its owned rows only and leaves the
     * rest of `data` alone); padding rows are written as zeros and never returned.  Writing b makes F stale, as new loads do. */
    FEMSHELL_KRYLOV_X = 0, FEMSHELL_KRYLOV_R = 1, FEMSHELL_KRYLOV_Z = 2, FEMSHELL_KRYLOV_P = 3, FEMSHELL_KRYLOV_Q = 4,
    FEMSHELL_KRYLOV_SV = 5, FEMSHELL_KRYLOV_B = 6,
    FEMSHELL_KRYLOV_PARTIALS = 7, /* the partial-sum arrays as raw words: n <= 4 G doubles from the start, G = femshell_krylov_grid */
    FEMSHELL_KRYLOV_SCALARS = 8,  /* one femshell_krylov_scalars (n = its size in doubles) */
    FEMSHELL_KRYLOV_HISTORY = 9,  /* the history buffer of the probe, its own: set allocates n <= 4096 words, fills them and makes n
                                   * the cap; get reads n <= that many */
    FEMSHELL_KRYLOV_HISTORY_CAP = 10 /* data[0]: the cap the launches see, 0 .. the words of the buffer (words beyond stay as set) */
};
enum {
    FEMSHELL_KSTEP_CG_INIT = 0,         /* args[0]: restart */
    FEMSHELL_KSTEP_CG_UPDATE = 1,       /* args[0]: gather (symmetric storage) */
    FEMSHELL_KSTEP_CG_DIRECTION = 2,
    FEMSHELL_KSTEP_CGCG_INIT = 3,
    FEMSHELL_KSTEP_CGCG_UPDATE = 4,     /* args[0]: step -1, 0 or 1; args[1]: gather */
    FEMSHELL_KSTEP_PCG_INIT = 5,
    FEMSHELL_KSTEP_PCG_UPDATE = 6,
    FEMSHELL_KSTEP_PCG_UPDATE_START = 7, /* args[0]: gather.  Multigrid contexts with a built hierarchy of two levels or more; the
                                          * direction goes to level 0's d vector, the iterate to z */
    FEMSHELL_KSTEP_PCG_NORM = 8,
    FEMSHELL_KSTEP_PCG_DOTS = 9,
    FEMSHELL_KSTEP_MINV_APPLY_NORM = 10, /* z = D^-1 q, partial sums of z.z */
    FEMSHELL_KSTEP_PRODUCT = 11,        /* spmv_with_halo: args[0] = 0: q = K p, sums from partials[0]; 1: q = K z, sums from
                                         * partials[2 G] (single-reduction); args[1]: the gather is left to the next kernel.
                                         * iout[0] = the partial sums it reports (0: G) */
    FEMSHELL_KSTEP_SYM_GATHER = 12,     /* q += the transposed products (symmetric storage) */
    FEMSHELL_KSTEP_TWO_DOTS = 13,       /* args[0], args[1]: two of the vectors above, 0 .. 6: dout = (a.a, b.b) */
    FEMSHELL_KSTEP_SCALAR_STEP = 14,    /* scalar_step: args = nsums, phase, n_partials (0: G), len3, gate_phase (-1: the phase's) */
    FEMSHELL_KSTEP_PC_APPLY = 15,       /* z = M(r) as the flexible recurrence issues it, gated by the scalars; args[0]: the first
                                         * pre-smoothing step was taken by PCG_UPDATE_START.  Multigrid contexts with a hierarchy */
    FEMSHELL_KSTEP_COPY_Z_TO_P = 16     /* p = z, gated by the scalars (the first direction of the flexible recurrence) */
};
int32_t femshell_krylov_grid(femshell_ctx *ctx); /* workgroups of the per-slice kernels = partial sums per array; -1 without a mesh */
int femshell_krylov_set(femshell_ctx *ctx, int32_t which, const double *data, int64_t n);
int femshell_krylov_get(femshell_ctx *ctx, int32_t which, double *data, int64_t n);
/* Exactly one production launch (PRODUCT, TWO_DOTS, SCALAR_STEP, PC_APPLY: the production sequence of that name) on that state,
 * then a stream synchronisation and hipGetLastError.  args: five words (unused ones 0); iout (two words) and dout (two doubles)
 * may be NULL where the step returns nothing. */
int femshell_krylov_launch(femshell_ctx *ctx, int32_t step, const int32_t *args, double rtol, int32_t *iout, double *dout);
/* launch_cg_scalar(reduce, phase NONE) on the caller's arrays, in a buffer of this call alone and with scalars of the probe's own,
 * kept from call to call as a solve keeps its: partials holds nsums (1 .. 3) arrays of n_partials (1 .. 2^20) doubles one behind the
 * other, the third of them len3 (1 .. n_partials) long.  red_out[3]: the sums (NaN where the launch wrote none); *ticket_out: the
 * arrival counter behind the launch.  Needs no mesh. */
int femshell_cg_reduce(femshell_ctx *ctx, int32_t n_partials, int32_t nsums, int32_t len3, const double *partials, double *red_out,
                       uint32_t *ticket_out);
/* ---- For tests: the block kernels of the eigen-solvers one launch at a time (csrc/api_modal_probe.cpp): those
 * of csrc/modal.hip that otherwise run only inside femshell_modes / femshell_buckling.  Each call uploads its blocks (columns of
 * n_nodes x 6 doubles in the caller's numbering, one behind the other) into device buffers of its own, calls the production
 * launcher once and downloads; nothing the context keeps is written, no production path runs through these.  Every output buffer
 * is filled with bytes that read as NaN before the launch: a row the kernel does not write comes back as NaN.  *stray: the 8-byte
 * words in the rows behind the owned ones (the padding of every output column) that are not +0.0 bit for bit.  One rank only
 * (FEMSHELL_ERR_UNSUPPORTED for a row-partitioned context); FEMSHELL_ERR_INVALID without a mesh, the context as it was. */
/* Y = sum_k S[k] C_k (k_block_combine): n_src (1 .. 3) sources of q[k] (0 .. 96, not all 0) columns, S[k] may be NULL where q[k] = 0;
 * C: (sum q) x ldc row-major, the rows of source k behind those of source k - 1; Y: n_out (1 .. 64, <= ldc) columns. */
int femshell_modal_combine(femshell_ctx *ctx, int32_t n_src, const int32_t *q, const double *const *S, const double *C, int32_t ldc,
                           int32_t n_out, double *Y, int64_t *stray);
/* R_i = KX_c - theta[c] m o X_c, c = cols[i], on the free dofs (k_block_residual, k_block_residual_sums; m: the lumped mass, so a
 * density must be set): KX, X: mb (1 .. 96) columns, theta[mb], cols[n] (n 1 .. 96, each in 0 .. mb - 1).  R: n columns;
 * norms[n]: sum r^2 / m; partials (may be NULL): n x 128, the partial sums of every column as the first kernel left them. */
int femshell_modal_residual(femshell_ctx *ctx, int32_t mb, const double *KX, const double *X, const double *theta, int32_t n,
                            const int32_t *cols, double *R, double *norms, double *partials, int64_t *stray);
/* Z = D^-1 R masked on the constrained dofs (k_block_bj), n (1 .. 96) columns; assembles K and builds its block-Jacobi inverse
 * where they are missing (the inverse femshell_block_jacobi_export shows at level 0).  Not while dynamics is active. */
int femshell_modal_block_jacobi(femshell_ctx *ctx, int32_t n, const double *R, double *Z, int64_t *stray);
/* X = mask(X) in place (k_block_mask), n (1 .. 96) columns */
int femshell_modal_mask(femshell_ctx *ctx, int32_t n, double *X, int64_t *stray);
/* the hashed start vectors of femshell_modes (k_modal_init), n_cols (1 .. 96) columns, with the node numbering femshell_modes
 * passes: the context's permutation, or none */
int femshell_modal_start(femshell_ctx *ctx, int32_t n_cols, double *X, int64_t *stray);
/* The device-memory pool of this process as it stands (csrc/dev_pool.hpp; every buffer of every context comes out of it, so the
 * call takes no context and also answers after the last one was destroyed): out[0] = bytes the driver has handed out through
 * the pool and not got back, out[1] = bytes in use by buffers, out[2] = bytes kept for reuse (what FEMSHELL_POOL_GB bounds),
 * out[3] = arenas (blocks that requests are carved from), out[4] = the bytes in them, out[5] = blocks that wait for the end of
 * a multigrid setup.  The counters are the pool's own; all six are zero once the last context is gone. */
int femshell_pool_stats(double out[6]);
/* Multigrid hierarchy of a row-partitioned context (the reference's PETSc preconditioner lives on the distributed matrix,
 * doc/implementation.tex:463-472): out[0] = levels whose rows are split over the ranks (0: single-rank context), out[1] =
 * bytes of this rank's operators on those levels (they shrink with the rank count), out[2] = bytes of the levels below,
 * which every rank holds in full (dense inverse included), out[3] / out[4] = this rank's rows / ghost rows on the last
 * row-partitioned level, out[5] = nodes of the first replicated level. */
int femshell_amg_partition_info(femshell_ctx *ctx, double out[6]);
/* Algorithmic HBM bytes of ONE multigrid cycle (one application of the preconditioner inside femshell_solve, which replaces the
 * PETSc preconditioner behind equation_systems.solve(), fem-shell.cpp:138), level by level: per_level[l] = what the cycle streams on
 * level l over all its visits per outer iteration -- smoothing products on the single-precision copies where the level keeps them,
 * residual increments, transfers, the K cycle's FP64 products, the dense solve of the coarsest level (csrc/amg_solve.cpp
 * amg_cycle_bytes spells the model out).  Returns the number of levels (< 0: error); at most `cap` entries are written.
 * femshell_solve_info::bytes_per_iteration = their sum + the Krylov method's own passes on level 0. */
int32_t femshell_amg_cycle_bytes(femshell_ctx *ctx, double *per_level, int32_t cap);
/* which assembly kernel femshell_assemble launches for the mesh of this context (after femshell_set_mesh): 1 = the
 * pipelined one (k_assemble_pipe: meshes whose slices touch at most 150 elements -- 77 with quadrilaterals -- and whose
 * work items fit one round of its waves: structured meshes, unstructured ones numbered with locality), 0 = the two-phase
 * one (k_assemble: scattered numberings, full storage, FEMSHELL_ASM_PIPE=0); < 0: error.  Same results either way. */
int femshell_assembly_kernel(femshell_ctx *ctx);

/* replaces: equation_systems.solve() -> PETSc KSPSolve (SA:138, PC:271) followed by
 * build_solution_vector (SA:141; PC:274-280 broadcast): 6x6-block-Jacobi preconditioned CG,
 * x0 = 0 (or what femshell_set_initial_guess handed over for this solve), stop at ||r||_2 <= rtol*||b||_2 or max_it.
 * rtol <= 0 runs exactly max_it iterations.
 * u_out[n_nodes][6] receives the full solution on every rank; NULL leaves it in HBM
 * (fetch with femshell_get_solution).  Assembles first if needed.
 * Contexts with a communicator (femshell_comm_init) run the single-reduction form of the same method
 * (Chronopoulos & Gear: one all-reduce of r.z, r.r, z.Az per iteration); the iterates agree with the classic
 * recurrence up to rounding.  FEMSHELL_CG_SINGLE_REDUCTION=0/1 in the environment overrides the choice. */
int femshell_solve(femshell_ctx *ctx, double rtol, int32_t max_it, double *u_out,
                   femshell_solve_info *info);
int femshell_get_solution(femshell_ctx *ctx, double *u_out);
/* extends: the reference writes displacements only (SA:141-169); this gives what the supports carry.
 *     r = K_unc u - loads
 * with the unconstrained stiffness (the element product of femshell_set_prescribed) and the loads as set, NOT masked.  At free
 * dofs r is the negative residual of the solve; at fixed dofs it is the support reaction: force (u, v, w) and moment (tx, ty,
 * tz) the support exerts on the shell.  The translations are in the null space of K_unc, so the force columns of r summed over
 * all nodes balance the summed loads.  u: n_nodes x 6 in the caller's numbering, or NULL: the solution of the last solve,
 * prescribed part included (taken where it lies in HBM).  r6_out: n_nodes x 6, the caller's numbering (FEMSHELL_REORDER too).
 * Needs a mesh, not an assembled K.  Sums in a fixed order: two calls give the same bits, and the NULL form gives the bits of the
 * explicit one.  FEMSHELL_ERR_UNSUPPORTED on a row-partitioned context (world_size != 1). */
int femshell_reactions(femshell_ctx *ctx, const double *u /* n_nodes x 6, or NULL */, double *r6_out /* n_nodes x 6 */);
/* extends: the reference writes displacements only, and its thesis names the stresses as future work; this gives what the shell
 * carries.  Per element 14 doubles, rows in the caller's order: its triangles, then its quadrilaterals (FEMSHELL_REORDER too):
 *     [0..5]   membrane force tensor N (force per length), global axes, order xx, yy, zz, xy, yz, zx
 *     [6..11]  moment tensor M (moment per length), global axes, same order
 *     [12]     von Mises stress at the top surface (z = +t/2 along the element's local z axis), [13] at the bottom surface
 * In the element frame (the one K is built with) N_loc = t Dm eps and M_loc = -Dp kappa, so that M = integral of sigma z dz, with
 * eps = (u,x, v,y, u,y + v,x) and kappa = (w,xx, w,yy, 2 w,xy) the ELEMENT MEANS of the element's own strain operators by the
 * quadrature its stiffness uses: TRI3 the constant CST strain and the mean of Specht's curvature over its three Gauss points (the
 * same Y as the stiffness, FEMSHELL_REF_Y21 included), QUAD4 the det-J-weighted mean over the 2 x 2 Gauss points of the bilinear
 * membrane strain and the DKQ curvature.  The tensors are R^T [[a_xx, a_xy, 0], [a_xy, a_yy, 0], [0, 0, 0]] R (rows of R: the
 * local axes), which does not depend on the in-plane axes an element happens to choose.  sigma_top/bottom = N_loc / t +- 6 M_loc / t^2,
 * von Mises in its plane-stress form; with sections t, Dm, Dp are the element's own.  The drilling rotation carries no resultant;
 * Kirchhoff elements have no transverse shear.
 * u: n_nodes x 6 in the caller's numbering, or NULL: the solution of the last solve, prescribed part included (taken where it
 * lies in HBM).  Needs a mesh, not an assembled K.  No sums across elements: two calls give the same bits, and the NULL form gives
 * the bits of the explicit one.  A degenerate element: FEMSHELL_ERR_MESH.  FEMSHELL_ERR_UNSUPPORTED on a row-partitioned context
 * (world_size != 1); FEMSHELL_ERR_INVALID while dynamics is active, without a mesh, for the NULL form before any solve, for a
 * non-finite u.  The context stays usable after every refusal. */
int femshell_element_resultants(femshell_ctx *ctx, const double *u /* n_nodes x 6, or NULL */, double *out /* (n_tri + n_quad) x 14 */);
/* extends: the element means above, averaged to the nodes, and how far each element lies from that average in the energy norm
 * (the Zienkiewicz-Zhu indicator).  Tensors are six words xx, yy, zz, xy, yz, zx in global axes, as above.
 *     T:T = xx^2 + yy^2 + zz^2 + 2 (xy^2 + yz^2 + zx^2),  tr T = xx + yy + zz
 *     q_nu(S, T) = (1 + nu) S:T - nu tr S tr T        (frame-free; for tangent tensors the plane-stress compliance times E)
 *     cN(S, T) = q_nu(S, T) / (E t),  cM(S, T) = 12 q_nu(S, T) / (E t^3)       (E, nu, t the element's own: its section's)
 *     a_e: the vector area of the element, TRI3 (b-a) x (c-a) / 2, QUAD4 d1 x d2 / 2 (d1 = c-a, d2 = d-b);  A_e = |a_e|, the
 *     area of femshell_lumped_mass and of the element loads
 * nodes_out, per node 14 doubles, rows in the caller's numbering (FEMSHELL_REORDER too):
 *     [0..5]   N* = sum_e A_e N_e / W,  [6..11]  M* = sum_e A_e M_e / W  over the elements e that contain the node, N_e and M_e
 *              the words 0..11 of the element's row of femshell_element_resultants (prescribed values and temperatures in force
 *              included)
 *     [12]     W = sum_e A_e
 *     [13]     the fold measure 1 - |sum_e a_e| / W: 0 where the neighbourhood is flat and consistently oriented, 1 - cos(phi/2)
 *              on a fold of angle phi between equal areas, 1 where orientations cancel.  M changes sign with an element's node
 *              order: the measure tells where the average means nothing.
 *     W = 0: fourteen zeros.
 * elems_out, per element 2 doubles, rows in the caller's order (triangles, then quadrilaterals), with
 * d_i = (N*_i - N_e, M*_i - M_e) at the element's corners and c(d_i, d_j) = cN(.,.) + cM(.,.):
 *     [0]      e2 = A_e c(sigma_e, sigma_e): twice the complementary energy of the element means
 *     [1]      eta^2 = A_e sum_ij w_ij c(d_i, d_j), the exact integral of the interpolated difference: TRI3 w_ij = (1 + delta_ij) / 12;
 *              QUAD4 w = 4/36 for the same corner, 2/36 for corners that share a side, 1/36 for the diagonal (the bilinear mass
 *              of a parallelogram, used as the definition on any quadrilateral)
 * The relative error of a mesh is sqrt(sum eta^2 / (sum e2 + sum eta^2)), summed by the caller.
 * KNOWN LIMIT: at folds and where the section changes the jump of N and M is physical; the indicator reports it as error.  The
 * fold measure and the section ids let a caller mask those nodes (smoothing groups are an open end).
 * Either output may be NULL, not both.  u as for femshell_element_resultants, and the same refusals: FEMSHELL_ERR_UNSUPPORTED on a
 * row-partitioned context; FEMSHELL_ERR_INVALID while dynamics is active, without a mesh, for the NULL form before any solve, for
 * a non-finite u, for two NULL outputs; a degenerate element: FEMSHELL_ERR_MESH.  The sums of a node run over its elements in a
 * fixed order without atomics: two calls give the same bits.  Nothing is kept: the context is as it was. */
int femshell_nodal_resultants(femshell_ctx *ctx, const double *u /* n_nodes x 6, or NULL */, double *nodes_out /* n_nodes x 14, or NULL */,
                              double *elems_out /* (n_tri + n_quad) x 2, or NULL */);
/* The NEXT femshell_solve of this context starts from u0 (n_nodes x 6, the caller's numbering; every rank passes the whole vector
 * and keeps its own rows) instead of from zero; u0 == NULL: from the solution of the context's previous solve, where it lies in
 * HBM (no transfer).  Consumed by that solve; femshell_set_mesh forgets it.
 * replaces: libMesh hands system.solution to KSPSolve as the initial guess (PetscLinearSolver: KSPSetInitialGuessNonzero), so
 * every equation_systems.solve() of the coupled adapter's loop (fem-shell_precice.cpp:271) starts from the displacements of the
 * last coupling iteration; the stand-alone program's one solve (fem-shell.cpp:138) starts from zero either way.
 * The stopping rule is unchanged (||r|| <= rtol ||b||, the refinement passes of the multigrid-preconditioned solve and their
 * error estimate): the first phase solves the correction equation K e = b - K u0, its right-hand side evaluated in
 * double-double, down to the threshold a solve from zero runs to.  Block-Jacobi: classic recurrence from r = b - K u0. */
int femshell_set_initial_guess(femshell_ctx *ctx, const double *u0);
/* ||r||/||b|| after each iteration of the last solve; returns the count written (<= cap) */
int32_t femshell_residual_history(femshell_ctx *ctx, double *hist, int32_t cap);

/* ---- structural dynamics: lumped mass and Newmark time stepping ------------------------
 * extends: the reference treats every load as static (its thesis names a mass matrix, a damping matrix and nodal velocities and
 * accelerations as future development; the coupled adapter's time loop, PC:271, is a fresh static solve per step).
 *
 * Mass density.  n_sections == 0: `rho` is the density of the whole shell (paired with the thickness of the femshell_config, or with
 * every section's own thickness when the context has sections).  Otherwise n_sections must equal the section count of the context
 * and section_rho[s] is the density of section s.  Every density must be finite and > 0; FEMSHELL_ERR_INVALID leaves the densities
 * that were in force untouched.  femshell_set_mesh and femshell_set_sections forget the densities.
 *
 * The mass matrix M is LUMPED (diagonal): a TRI3 element of area A = |(b-a) x (c-a)| / 2 gives each of its three nodes
 * rho t A / 3 on u, v, w and rho t^3/12 A / 3 on tx, ty, tz; a QUAD4 with diagonals d1, d2 has A = |d1 x d2| / 2 and gives a quarter
 * of rho t A and of rho t^3/12 A to each of its four nodes.  Both parts are multiples of the identity per node: M needs no
 * local-to-global rotation and is positive definite on every dof, rotations and drilling included.  The sums run over the
 * elements in a fixed order without atomics: M is bitwise reproducible, like K. */
int femshell_set_density(femshell_ctx *ctx, double rho, int32_t n_sections, const double *section_rho);
/* m6_out[n_nodes][6]: the diagonal of M in the caller's numbering, NOT masked by the Dirichlet set; on a row-partitioned context
 * every rank receives all rows (gathered like the solution). */
int femshell_lumped_mass(femshell_ctx *ctx, double *m6_out);

/* Newmark's method with mass-proportional damping C = alpha M:  M a + C v + K u = F(t).
 *   a0 = 1/(beta dt^2), a1 = gamma/(beta dt), a2 = 1/(beta dt), a3 = 1/(2 beta) - 1, a4 = gamma/beta - 1, a5 = dt/2 (gamma/beta - 2)
 *   K_eff = K + (a0 + alpha a1) M on the free dofs (constrained rows keep what the assembly wrote)
 *   F_eff = mask(F_{n+1} + M [(a0 u + a2 v + a3 a) + alpha (a1 u + a4 v + a5 a)]),  K_eff u' = F_eff
 *   a' = a0 (u' - u) - a2 v - a3 a,  v' = v + dt [(1 - gamma) a + gamma a']
 *   initial acceleration on the free dofs: M^-1 (F_0 - alpha M v_0 - K u_0);  u, v, a are 0 on constrained dofs.
 * Only the unconditionally stable schemes are accepted: dt > 0, gamma >= 1/2, beta >= (gamma + 1/2)^2 / 4, alpha >= 0.
 *
 * femshell_dynamics_begin (u0, v0: n_nodes x 6 in the caller's numbering, every rank passes the whole vectors; NULL = 0) assembles
 * K if needed, computes the initial acceleration from the loads in force and adds the shift to the diagonal of K in HBM.
 * WHILE DYNAMICS IS ACTIVE THE MATRIX IN HBM IS K_eff: femshell_export_bsr, femshell_spmv, femshell_residual and femshell_solve
 * see K_eff; block-Jacobi and the multigrid hierarchy are built from it at the first step (once per dt).  femshell_set_loads
 * stays allowed (F_{n+1} of the next step); femshell_set_dirichlet, femshell_set_sections, femshell_set_density and a second
 * femshell_dynamics_begin return FEMSHELL_ERR_INVALID; femshell_set_mesh ends dynamics.
 *
 * femshell_dynamics_step solves for the CANDIDATE state (u', v', a') of the step from the committed state to t + dt, the solve
 * started from the committed u; calling it again without femshell_dynamics_accept recomputes the candidate from the same committed
 * state (the iteration checkpoint of an implicit coupling), bit for bit when nothing changed.  femshell_dynamics_accept commits
 * the candidate.  femshell_get_solution returns the last candidate u.  femshell_dynamics_state copies out u, v, a (each
 * n_nodes x 6 or NULL; which = 0: committed, 1: candidate), gathered to every rank like the solution.  femshell_dynamics_energy:
 * out[0] = v.M v / 2, out[1] = u.K u / 2 (the K without the shift), sums in a fixed order.  femshell_dynamics_end drops the
 * state; K and F are assembled again at the next use and a static solve is what a fresh context gives. */
typedef struct femshell_dynamics_options { double dt, beta, gamma, alpha; } femshell_dynamics_options;
int femshell_dynamics_defaults(femshell_dynamics_options *out); /* beta 1/4, gamma 1/2, alpha 0, dt 0 (to be set) */
int femshell_dynamics_begin(femshell_ctx *ctx, const femshell_dynamics_options *opt, const double *u0, const double *v0);
int femshell_dynamics_step(femshell_ctx *ctx, double rtol, int32_t max_it, femshell_solve_info *info);
int femshell_dynamics_accept(femshell_ctx *ctx);
int femshell_dynamics_state(femshell_ctx *ctx, int32_t which, double *u, double *v, double *a);
int femshell_dynamics_energy(femshell_ctx *ctx, int32_t which, double out[2]);
int femshell_dynamics_end(femshell_ctx *ctx);

/* ---- modal analysis: natural frequencies and mode shapes ----------------------------------------------------------------
 * extends: the reference has no eigenvalue analysis; with the lumped mass M of femshell_set_density this solves
 *     K x = lambda M x,  lambda = omega^2,
 * on the free dofs for the n_modes lowest pairs, by LOBPCG on the device (csrc/modal.cpp) with a block of
 * mb = n_modes + guard vectors, preconditioned by what femshell_set_preconditioner chose: one multigrid cycle per column, or
 * the 6x6 block-Jacobi inverse.  The products with K multiply four columns per pass over the stored blocks (k_spmm_sym,
 * csrc/modal.hip) with symmetric storage, and go column by column through the single-vector kernel with full storage.
 *
 * Pair j has converged when ||K x_j - lambda_j M x_j||_{M^-1} <= tol (lambda_j + shift) with x_j^T M x_j = 1; the call stops when
 * the n_modes lowest pairs have, or after max_it iterations: it then returns FEMSHELL_OK with info->converged < n_modes and the
 * best pairs it has.  shift >= 0 solves the pencil (K + shift M) x = (lambda + shift) M x -- the shift is added to the free
 * diagonal of K in HBM as femshell_dynamics_begin adds its own, the preconditioner is built from the shifted matrix, lambda is
 * reported with the shift subtracted -- which is what makes an unconstrained shell solvable (its K has the three rigid
 * translations in the null space).  After the call the shift is gone: K is assembled again at the next use, as after
 * femshell_dynamics_end.  A K + shift M that is not positive definite surfaces as FEMSHELL_ERR_BREAKDOWN (a host-side test of
 * the Ritz values x.(K + shift M)x and of the Gram matrices; the message names `shift`).
 *
 * lambda_out[n_modes] ascending; modes_out (n_modes x n_nodes x 6, the caller's numbering, or NULL): M-orthonormal, each with the
 * sign that makes its entry of largest magnitude positive (lowest index on ties); residual_out[n_modes] (or NULL):
 * ||K x - lambda M x||_{M^-1} / (lambda + shift).  Two calls on the same context give the same bits (start vectors are a hash of
 * the caller's node id, dof and column; every sum has a fixed order).
 * FEMSHELL_ERR_INVALID, the context left as it was: no mesh, no density, n_modes < 1, guard < 0, n_modes + guard > 32, fewer than
 * 3 (n_modes + guard) free dofs, tol <= 0, shift < 0, max_it < 1, dynamics active.  FEMSHELL_ERR_UNSUPPORTED: a row-partitioned
 * context (world_size != 1). */
typedef struct femshell_modal_options { int32_t n_modes, guard, max_it, reserved; double tol, shift; } femshell_modal_options;
typedef struct femshell_modal_info {
    int32_t iterations, converged /* pairs */, block /* mb */, restarts, fused_product /* 1: k_spmm_sym ran */, pc_type;
    double residual_max;        /* worst ||Kx - lambda Mx||_{M^-1} / (lambda + shift) of the returned pairs */
    double seconds_total, seconds_product, seconds_precond, seconds_gram, seconds_update, pc_setup_seconds;
} femshell_modal_info;
int femshell_modal_defaults(femshell_modal_options *out);   /* n_modes 6, guard 4, max_it 500, tol 1e-6, shift 0 */
int femshell_modes(femshell_ctx *ctx, const femshell_modal_options *opt, double *lambda_out /* n_modes */,
                   double *modes_out /* n_modes x n_nodes x 6, or NULL */, double *residual_out /* n_modes, or NULL */,
                   femshell_modal_info *info);
/* ---- geometric (initial-stress) stiffness ------------------------------------------------------------------------------------
 * extends: the reference has no stability analysis; this is the operator linear buckling adds to K, (K + lambda K_G) x = 0.
 *
 * Prestress.  The prestress of an element is its element-mean membrane force N_loc = (Nxx, Nyy, Nxy) of
 * femshell_element_resultants, from the displacement vector u (n_nodes x 6, the caller's numbering), or u == NULL: from the solution
 * of the last solve, prescribed part included.  The element's own section applies.
 * Element matrix.  With phi_a the membrane shape functions in the element frame's in-plane coordinates -- TRI3: linear, one point
 * of weight A; QUAD4: bilinear, at the stiffness's 2 x 2 Gauss points with weight det J --
 *     g_ab = sum_gp w_gp grad phi_a(gp)^T [[Nxx, Nxy], [Nxy, Nyy]] grad phi_b(gp)      (symmetric; rows sum to 0)
 *     K_G,e[a, b] = g_ab I3 on the translations (u, v, w), zero on the three rotations:
 * the full Green-Lagrange term on all three translations, which needs no local-to-global rotation and gives a rigid translation
 * zero geometric energy.  K_G is never stored: the unique g_ab of every element (6 or 10 doubles) are, and the product walks the
 * slices' element lists (csrc/geometric_stiffness.hip).
 *
 * femshell_geometric_product: Y = K_G(u) X, UNCONSTRAINED (whatever femshell_set_dirichlet holds), for n_cols (1 .. 96) columns of
 * n_nodes x 6 in the caller's numbering, column j at X + j * n_nodes * 6.  The rotational rows are exactly zero.  Needs a mesh
 * only.  The additions of a row run in the order of its slice's element list, without atomics: two calls give the same bits,
 * column j of a block is bitwise the single-column product, and the NULL form gives the bits of the explicit one.  A degenerate
 * element: FEMSHELL_ERR_MESH.  FEMSHELL_ERR_UNSUPPORTED on a row-partitioned context (world_size != 1); FEMSHELL_ERR_INVALID
 * while dynamics is active, without a mesh, for the NULL form before any solve, for a non-finite u, for n_cols out of range.  The
 * context stays usable after every refusal. */
int femshell_geometric_product(femshell_ctx *ctx, const double *u /* n_nodes x 6, or NULL */, int32_t n_cols /* 1 .. 96 */,
                               const double *X, double *Y);

/* ---- linear buckling: load factors and buckling shapes ------------------------------------------------------------------
 * extends: the reference has no stability analysis; with the geometric stiffness above this solves the pencil
 *     (K + lambda K_G(u)) x = 0
 * on the free dofs of the Dirichlet set: at lambda times the load that produced u the shell buckles in the shape x.  Returned are
 * the n_modes factors of SMALLEST MAGNITUDE, SIGNED, ordered by |lambda|, a positive one before a negative one of equal magnitude.
 * A negative factor means the shell buckles under the reversed load; shear gives +- pairs.  (Magnitudes that agree to `tol` count
 * as equal: the two members of such a pair differ by rounding only.)
 *
 * Method (csrc/buckling.cpp): block inverse iteration with Rayleigh-Ritz on A x = mu K x, A = -K_G, mu = 1 / lambda, with a block
 * of mb = n_modes + guard columns: mb solves with K per iteration by the context's CG and preconditioner (femshell_set_preconditioner),
 * the block product of femshell_modes, k_geometric_product, the Gram kernel, Cholesky and Jacobi on the host.  Pair j has converged
 * when
 *     rho_j = ||A x_j - mu_j K x_j||_{K^-1} / (|mu_j| ||x_j||_K) <= tol
 * (some eigenvalue mu lies within rho_j |mu_j| of mu_j); the pairs returned have passed the test with a solve and products of their
 * own.  The inner solves run to the relative residual inner_rtol (0: tol / 100).  Reaching max_it returns FEMSHELL_OK with
 * info->converged < n_modes and the best pairs the call has.
 *
 * u: the displacements whose membrane forces are the prestress (n_nodes x 6), or NULL: the solution of the last solve, prescribed
 * part included.  lambda_out[n_modes]; modes_out (n_modes x n_nodes x 6, the caller's numbering, or NULL): each scaled so that its
 * translational entry of largest magnitude is +1 (lowest index on ties); rho_out[n_modes] (or NULL).  Two calls give the same bits.
 * After the call the context is as it was: F, the last solution, a pending initial guess, K, block-Jacobi and the hierarchy (which
 * the call builds where they were not there; a breakdown of the multigrid-preconditioned solve under single-precision copies
 * rebuilds the hierarchy in FP64 as femshell_solve does).
 * FEMSHELL_ERR_BREAKDOWN: no prestress at all (K_G = 0), Gram matrices that are not finite, a Y^T K Y that is not positive
 * definite (K_G has too low a rank for the block: reduce n_modes + guard).  FEMSHELL_ERR_INVALID, the context left as it was: no
 * mesh, the NULL form before any solve, a non-finite u, n_modes < 1, guard < 0, n_modes + guard > 32, fewer than
 * 2 (n_modes + guard) free translational dofs, tol <= 0, inner_rtol < 0, max_it < 1, dynamics active.  FEMSHELL_ERR_UNSUPPORTED: a
 * row-partitioned context (world_size != 1). */
typedef struct femshell_buckling_options { int32_t n_modes, guard, max_it, reserved; double tol, inner_rtol; } femshell_buckling_options;
typedef struct femshell_buckling_info {
    int32_t iterations, converged /* pairs */, block /* mb */, pc_type;
    int64_t inner_iterations;   /* CG iterations of all inner solves */
    double rho_max;             /* worst rho of the returned pairs */
    double seconds_total, seconds_solves, seconds_products, seconds_gram, seconds_update;
} femshell_buckling_info;
int femshell_buckling_defaults(femshell_buckling_options *out);   /* n_modes 4, guard 4, max_it 100, tol 1e-8, inner_rtol 0 (tol / 100) */
int femshell_buckling(femshell_ctx *ctx, const femshell_buckling_options *opt, const double *u /* n_nodes x 6, or NULL */,
                      double *lambda_out /* n_modes */, double *modes_out /* n_modes x n_nodes x 6, or NULL */,
                      double *rho_out /* n_modes, or NULL */, femshell_buckling_info *info);

/* ---- load cases: several right-hand sides on one K ----------------------------------------------------------------------
 * extends: the reference solves one load per run (fem-shell.cpp:138); a structural job is a list of load cases on one model.
 *     K u_j = mask(loads_j),  j = 0 .. n_cases - 1  (1 <= n_cases <= 32),
 * from zero, with the K the context holds: sections and elastic supports included, the Dirichlet set with ZERO values.
 * loads: n_cases x n_nodes x 6 in the caller's numbering (FEMSHELL_REORDER too), case j at loads + j * n_nodes * 6.  A CASE'S
 * VECTOR IS THE WHOLE LOAD OF THAT CASE: the context's own nodal, element and thermal loads are NOT added.  Compose cases from
 * femshell_element_load_vector and femshell_thermal_load_vector, which return exactly such vectors.  u_out: the same layout.
 *
 * Block-Jacobi contexts (csrc/cases.cpp, cases.hip): the classic preconditioned CG of femshell_solve for every case ON ITS OWN
 * RECURRENCE -- one alpha, beta and done flag per column; this is not block CG -- in passes of four cases (fewer where the LDS of
 * the block product says so, and a narrower last pass).  Per iteration one pass over the stored blocks of K multiplies all
 * columns of the pass (k_spmm_sym with symmetric storage; column by column through the single-vector kernel with full storage:
 * info->fused_product says which), and the vector kernels read every node's D^-1 block once for all columns.  A finished case is
 * frozen: the result of a case -- u, iterations, residual -- is bit for bit what it is when the case is solved alone, in any
 * position of a pass, beside any company; partial sums are added in a fixed order without atomics: two calls give the same bits.
 * The sums are grouped differently from femshell_solve's, so u agrees with femshell_solve to rounding, not to the bit.
 * Multigrid contexts (femshell_set_preconditioner): the cases run one after another through the context's multigrid-preconditioned
 * CG, sharing K, the hierarchy and the transfers (fused_product = 0, passes = n_cases).
 *
 * Stopping rule per case, femshell_solve's: ||r_j|| <= rtol ||b_j||; rtol <= 0 runs exactly max_it iterations of every case; a case
 * with b_j = 0 returns zeros, 0 iterations, converged.  case_info[j] (or NULL): iterations, converged (1, 0: max_it reached, -1:
 * breakdown) and the recurrence's ||r|| / ||b||.  info (or NULL): the passes, the product, the preconditioner, the seconds of the
 * Krylov loops and the algorithmic bytes of one iteration of every case.
 * The context is left as it was: F, the last solution and its history, a pending initial guess and the refinement statistics stay;
 * K, block-Jacobi and, under multigrid, the hierarchy are brought up to date and kept.
 * A breakdown (p.Kp <= 0) in a case freezes that case with converged = -1; the others finish, all of u_out is written and the call
 * returns FEMSHELL_ERR_BREAKDOWN.
 * FEMSHELL_ERR_UNSUPPORTED on a row-partitioned context (world_size != 1).  FEMSHELL_ERR_INVALID, u_out not written: no mesh, a
 * NULL ctx, loads or u_out, n_cases out of 1 .. 32, max_it < 0, a non-finite load, dynamics active, prescribed displacements in
 * force (the cases use zero values at the fixed dofs; femshell_set_prescribed with n = 0 clears them).  The context stays usable
 * after every refusal. */
typedef struct femshell_case_info { int32_t iterations, converged; double rel_residual; } femshell_case_info;
typedef struct femshell_cases_info {
    int32_t passes, fused_product /* 1: k_spmm_sym ran */, pc_type, reserved;
    double solve_seconds, bytes_per_iteration;
} femshell_cases_info;
int femshell_solve_cases(femshell_ctx *ctx, int32_t n_cases, const double *loads /* n_cases x n_nodes x 6 */, double rtol, int32_t max_it,
                         double *u_out /* n_cases x n_nodes x 6 */, femshell_case_info *case_info /* n_cases, or NULL */,
                         femshell_cases_info *info /* or NULL */);

/* ---- load combinations: the stress envelope over factored sums of cases ----------------------------------------------------
 * extends: the reference has no load cases; a structural check wants, per element, the worst stress and the extreme principal
 * forces and moments over all combinations sum_j f_cj (case j), and the combination that governs.
 * With u_j the caller's vector of case j (the layout of femshell_solve_cases' u_out), eps and kappa the element means of
 * femshell_element_resultants (same operators, same quadrature, the element's own section), in the element frame K is built with:
 *     T_j[e] = (Nxx, Nyy, Nxy, Mxx, Myy, Mxy),  N_loc = t Dm (eps(u_j) - tau_j eps0),  M_loc = -Dp (kappa(u_j) - tau_j kappa0)
 *     T_c[e] = sum_j f_cj T_j[e]                 (j = 0 .. n_cases - 1, in index order)
 * eps0, kappa0: the free thermal state of the temperatures in force (femshell_set_thermal); tau_j = case_thermal[j]: the multiple
 * of that state case j was loaded with -- 1 for a case composed from femshell_thermal_load_vector, 0 otherwise (NULL: all zero).
 * From T_c six values per element, none of which depends on the in-plane axes the element chooses:
 *     q0, q1 = von Mises (plane-stress form) of N/t + 6M/t^2 (top) and N/t - 6M/t^2 (bottom)
 *     q2, q3 = N1 >= N2, the principal membrane forces (Nxx+Nyy)/2 +- sqrt(((Nxx-Nyy)/2)^2 + Nxy^2)
 *     q4, q5 = M1 >= M2, the principal moments, likewise (their signs follow the element's node order, as M's do)
 *     env_out[e] = (max_c q0, max_c q1, max_c q2, min_c q3, max_c q4, min_c q5)
 * gov_out[e][k] (or NULL): the lowest combination index, from 0, that attains env_out[e][k].  Rows are the caller's elements,
 * triangles then quadrilaterals, under FEMSHELL_REORDER too.  A case's vector is taken whole: the context's prescribed values are
 * not added.  factors: n_combos x n_cases, row-major.  1 <= n_cases <= 32, 1 <= n_combos <= 256.
 * The call needs a mesh, not an assembled K; nothing is kept and nothing of the context changes.  Two calls give the same bits; a
 * combination's values do not depend on its position or on the other combinations, a case's contribution not on its position or
 * on the other cases; a factor of exactly 0 leaves no trace of its case.
 * info (or NULL): the device seconds of the two kernels and their algorithmic bytes.
 * FEMSHELL_ERR_UNSUPPORTED on a row-partitioned context.  FEMSHELL_ERR_INVALID, outputs not written: no mesh; a NULL ctx, u,
 * factors or env_out; counts out of range; a non-finite entry in u, factors or case_thermal; a non-zero case_thermal while no
 * temperatures are in force; dynamics active.  FEMSHELL_ERR_MESH: a degenerate element, named as femshell_element_resultants names
 * it.  The context stays usable after every refusal. */
typedef struct femshell_envelope_info {
    double seconds_cases, seconds_envelope;   /* device seconds of the two kernels */
    double bytes_cases, bytes_envelope;       /* algorithmic byte model, DESIGN.md 8n */
} femshell_envelope_info;
int femshell_combination_envelope(femshell_ctx *ctx, int32_t n_cases, const double *u /* n_cases x n_nodes x 6 */,
                                  const double *case_thermal /* n_cases, or NULL: zeros */,
                                  int32_t n_combos, const double *factors /* n_combos x n_cases, row-major */,
                                  double *env_out /* (n_tri + n_quad) x 6 */, int32_t *gov_out /* (n_tri + n_quad) x 6, or NULL */,
                                  femshell_envelope_info *info /* or NULL */);

/* test entry: G = A^T diag(w) B (qa x qb, row-major) by the solver's Gram kernel; A, B: qa / qb columns of n_nodes x 6 in the
 * caller's numbering, 1 <= qa, qb <= 96; weighted != 0: w = the lumped mass (a density must be set), else w = 1.  Partial sums
 * are added in a fixed order: two calls give the same bits. */
int femshell_modal_gram(femshell_ctx *ctx, int32_t qa, const double *A, int32_t qb, const double *B, int32_t weighted, double *G);

/* ---- parity / debug exports (single-rank contexts) --------------------------------- */

/* element matrices in the reference's variable-major element ordering Ke(n*alpha+i, n*beta+j)
 * (SA:1105-1109), unconstrained, as localToGlobalTrafo leaves them.  Triangles are elements
 * [0,n_tri), quads [n_tri, n_tri+n_quad); the range must not mix the two kinds.
 * Ke_out: count x 324 (TRI3) or count x 576 (QUAD4) doubles. */
int femshell_element_matrices(femshell_ctx *ctx, int32_t first, int32_t count, double *Ke_out);

int64_t femshell_nnz_blocks(femshell_ctx *ctx); /* number of 6x6 blocks of K on this rank */
/* K as block CSR with sorted columns (vals: nnzb x 36 row-major) and F, after femshell_assemble -- what
 * system.matrix / system.rhs hold after the callback (SA:1230-1231).  A rank exports the node rows
 * [femshell_row_begin, femshell_row_end) it owns: rowptr has row_end - row_begin + 1 entries, colidx holds global
 * node ids, F has 6 entries per owned row (one rank: the whole matrix). */
int femshell_export_bsr(femshell_ctx *ctx, int32_t *rowptr, int32_t *colidx, double *vals, double *F);
/* y = K x on the device */
int femshell_spmv(femshell_ctx *ctx, const double *x, double *y);
/* y = K_unc x on the device: the product with the UNCONSTRAINED stiffness, formed from the element matrices (no Dirichlet rows,
 * whatever femshell_set_dirichlet holds; csrc/element_product.hip).  x, y: n_nodes x 6, the caller's numbering.  Single-rank
 * contexts (FEMSHELL_ERR_UNSUPPORTED otherwise); needs a mesh only, not an assembled K.  A degenerate element: FEMSHELL_ERR_MESH. */
int femshell_element_product(femshell_ctx *ctx, const double *x, double *y);
/* Y = K X for a block of n_cols (1 .. 96) vectors, column j at X + j * n_nodes * 6: the block product of femshell_modes; same
 * preconditions as femshell_spmv */
int femshell_spmm(femshell_ctx *ctx, int32_t n_cols, const double *X, double *Y);   /* Y = K X, columns of n_nodes x 6 */
/* r = F - K x with products and row sums in double-double (the residual the iterative refinement of the
 * multigrid-preconditioned solve restarts from); x[n_nodes][6] */
int femshell_residual(femshell_ctx *ctx, const double *x, double *r);

/* ---- row partition over several GPUs (one process per GPU, RCCL over xGMI) ---------- */

int32_t femshell_row_begin(femshell_ctx *ctx); /* first owned node row */
int32_t femshell_row_end(femshell_ctx *ctx);   /* one past the last owned node row */
/* The caller's ids of the node rows this rank owns, in the order femshell_export_bsr gives them; returns their number
 * (ids_out may be NULL).  Without a renumbering flag: row_begin .. row_end - 1.  With FEMSHELL_REORDER_MORTON / _RCM on a
 * row-partitioned context the library partitions the RENUMBERED rows (every rank computes the same permutation of the whole
 * mesh, then takes its stretch: a compact patch of the mesh whatever the caller's numbering is -- libMesh partitions its
 * elements for locality the same way, doc/implementation.tex:103-124), so the owned nodes are not a range of the caller's ids:
 * this list names them.  Node-indexed arguments (femshell_set_dirichlet, femshell_set_loads, the solution) keep the caller's
 * numbering on every rank. */
int32_t femshell_owned_nodes(femshell_ctx *ctx, int32_t *ids_out);
/* rank 0 creates the id, the host program distributes it (e.g. a torch.distributed or MPI
 * broadcast), every rank then calls femshell_comm_init before femshell_set_mesh.
 * replaces: LibMeshInit / init.comm() (SA:28, 35) */
int femshell_comm_unique_id(uint8_t id_out[128]);
int femshell_comm_init(femshell_ctx *ctx, const uint8_t id[128]);
/* ranks RCCL reports for this context's communicator (ncclCommCount); 0 when the context has none */
int32_t femshell_comm_ranks(femshell_ctx *ctx);
/* What femshell_comm_init checked on first contact, beyond the communicator itself: the communication patterns of a solve, once
 * each with a known answer and under the watchdog -- out_us[0]: a grouped ncclSend / ncclRecv ring on the halo stream beside an
 * ncclAllReduce of three words on the main stream (the reference's counterparts: PETSc's VecScatter halo and the MPI_Allreduce
 * inside KSPSolve, fem-shell.cpp:138); out_us[1]: grouped ncclBroadcast, one per rank (build_solution_vector + broadcast,
 * fem-shell.cpp:141, fem-shell_precice.cpp:277-280); out_us[2]: a lone all-reduce of three words.  Wall microseconds, enqueue
 * to completion.  Returns 1 when the self-test ran (a communicator exists), 0 when not (single-rank context), < 0 on error. */
int femshell_comm_selftest(femshell_ctx *ctx, double out_us[3]);
/* Communication this context has enqueued since the counters were last cleared: out[0] = grouped send/recv exchanges on the halo
 * stream (they run beside the interior slices of the product that needs them), out[1] = such exchanges on the main stream (in
 * the dependency chain: restrictions, prolongations, setup), out[2] = all-reduces, out[3] = grouped broadcasts (row gathers).
 * clear != 0 resets them.  What the reference leaves to PETSc (VecScatter, MPI_Allreduce inside KSPSolve, fem-shell.cpp:138) is
 * countable here: tests hold the per-iteration budget of the row-partitioned multigrid to these numbers.  Returns 1 with a
 * communicator, 0 without, < 0 on error. */
int femshell_comm_counters(femshell_ctx *ctx, int64_t out[4], int32_t clear);
/* ... and its volume: out[0] = bytes this rank handed to the sends of grouped exchanges (vector halos: 48 bytes per node another
 * rank reads; the multigrid setup: the rows of Q, P and A P of those nodes), out[1] = bytes it contributed to all-reduces and
 * broadcasts.  Same clearing and return values. */
int femshell_comm_bytes(femshell_ctx *ctx, int64_t out[2], int32_t clear);

/* ---- measurement ----------------------------------------------------------------- */

typedef enum femshell_kernel {
    FEMSHELL_KERNEL_ASSEMBLE = 0, /* element stiffness + block-row gather into K */
    FEMSHELL_KERNEL_SPMV = 1,     /* q = K p with fused p.q */
    FEMSHELL_KERNEL_CG_UPDATE = 2,/* x,r update + block-Jacobi apply + dots */
    FEMSHELL_KERNEL_CG_DIRECTION = 3, /* p = z + beta p */
    /* structural dynamics (a density must be set; the last three need femshell_dynamics_begin): launched back to back */
    FEMSHELL_KERNEL_LUMPED_MASS = 4,  /* k_lumped_mass */
    FEMSHELL_KERNEL_MASS_SHIFT = 5,   /* k_mass_shift (the shifts add up: K is assembled again at the next use) */
    FEMSHELL_KERNEL_NEWMARK_RHS = 6,  /* k_newmark_rhs */
    FEMSHELL_KERNEL_NEWMARK_UPDATE = 7, /* k_newmark_update (a candidate from whatever the solution vector holds; not committed) */
    /* modal analysis, launched back to back on scratch blocks of hashed vectors; FEMSHELL_TIME_KERNEL_COLS = c in the
     * environment (default 4, at most 32) sets the width */
    FEMSHELL_KERNEL_SPMM = 8,         /* Y = K X for c columns, both phases (FEMSHELL_SPMM_FUSED=0: column by column through
                                         the single-vector kernels, the yardstick of the fused kernel) */
    FEMSHELL_KERNEL_GRAM = 9,         /* S^T M S for 3c columns */
    FEMSHELL_KERNEL_BLOCK_COMBINE = 10, /* 2c columns out of 3c */
    /* k_element_product (y = K_unc x, matrix-free) back to back on a hashed vector; needs a mesh only.  bytes_out: coordinates,
     * the node ids of the slices' element lists, x read, y written */
    FEMSHELL_KERNEL_ELEMENT_PRODUCT = 11,
    /* k_element_resultants back to back on a hashed displacement vector; needs a mesh only.  bytes_out: 12 / 16 bytes of node ids
     * and 112 bytes of output per element (4 more of a section index where the context has sections), coordinates and
     * displacements (24 + 48 bytes) once per node */
    FEMSHELL_KERNEL_ELEMENT_RESULTANTS = 12,
    /* k_element_loads back to back on hashed element values, from the loads in force into a scratch vector; needs a mesh only, the
     * loads in force are not disturbed.  bytes_out: 16 bytes of node ids, 4 of element index and 32 of load words per entry of the
     * slices' element lists, 24 bytes of coordinates per node, 48 bytes of base read and 48 written per owned row */
    FEMSHELL_KERNEL_ELEMENT_LOADS = 13,
    /* k_geometric_product, one pass of four columns back to back on hashed coefficients and hashed vectors; needs a mesh only.
     * bytes_out: 16 bytes of node ids, 4 of element index and 48 (80 on a mesh with quadrilaterals) of coefficients per entry of
     * the slices' element lists, 24 bytes read and 48 written per owned row and column */
    FEMSHELL_KERNEL_GEOMETRIC_PRODUCT = 14,
    /* k_element_thermal back to back on hashed temperatures and a unit alpha, from the loads in force into a scratch vector; needs
     * a mesh only, the loads in force are not disturbed.  bytes_out: 16 bytes of node ids, 4 of element index and 16 of
     * temperatures per entry of the slices' element lists (4 more of a section index where the context has sections), 24 bytes
     * of coordinates per node, 48 bytes of base read and 48 written per owned row -- all six components carry a sum */
    FEMSHELL_KERNEL_ELEMENT_THERMAL = 15,
    /* k_nodal_recovery back to back on the element rows of a hashed displacement vector; needs a mesh only.  bytes_out: 16 bytes
     * of node ids, 4 of element index and 96 of tensor words per entry of the slices' element lists, 24 bytes of coordinates per
     * node, 112 bytes written per row of the slices (padding rows included) */
    FEMSHELL_KERNEL_NODAL_RECOVERY = 16,
    /* k_recovery_error back to back on the same rows and their nodal averages; needs a mesh only.  bytes_out: 12 / 16 bytes of
     * node ids, 96 of tensor words and 16 of output per element (4 more of a section index where the context has sections),
     * coordinates and recovered tensors (24 + 96 bytes) once per node */
    FEMSHELL_KERNEL_RECOVERY_ERROR = 17,
    /* k_support_rows back to back on hashed moduli into a scratch table; needs a mesh only, the table in force is not disturbed.
     * bytes_out: 16 bytes of node ids, 4 of element index and 16 of moduli per entry of the slices' element lists, 24 bytes of
     * coordinates per node, 72 bytes written per row of the slices (padding rows included) */
    FEMSHELL_KERNEL_ELASTIC_SUPPORT = 18
} femshell_kernel;

/* mean duration of one launch of the kernel from HIP events on the library's stream, over `reps` launches:
 * the assembly kernel back to back; a CG kernel inside `reps` iterations of the recurrence on scratch vectors
 * (this rank's rows, no communication), an event pair around that kernel of every iteration -- where it runs,
 * not back to back with itself.  bytes_out = algorithmic HBM bytes of one launch on this rank (DESIGN.md
 * section "algorithmic bytes").  The state of a solve is not disturbed. */
int femshell_time_kernel(femshell_ctx *ctx, femshell_kernel which, int32_t reps, double *mean_ms_out,
                         double *bytes_out);

/* hipStreamSynchronize on the library's stream */
int femshell_sync(femshell_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif
