// shell_system.hpp -- host-side mirror of the reference's program surface above the C ABI.
//
// The reference is a libMesh application: parameters are parsed into globals
// (fem-shell.h:42-52), an EquationSystems object owns a LinearImplicitSystem "Elasticity"
// with the callback assemble_elasticity attached (fem-shell.cpp:70-85), and
// equation_systems.solve() runs callback + Krylov solve (fem-shell.cpp:138).  libMesh, PETSc
// and preCICE do not exist in this image, so this C++ layer keeps the same names, argument
// meaning and error behaviour on top of libfemshell:
//
//   reference                                   here
//   read_parameters(argc, argv)   SA:194-267    femshell_host::read_parameters
//   mesh.read + "_f" file         SA:35-67      femshell_host::read_xda / read_forces
//   DirichletBoundary {0,20},{1,21} SA:90-120   ShellMesh::dirichlet_mask
//   assemble_elasticity(es, name) SA:1160-1233  ShellSystem::assemble_elasticity
//   equation_systems.solve()      SA:138        ShellSystem::solve
//   build_solution_vector(sols)   SA:141        ShellSystem::build_solution_vector
//
// The adaptor a libMesh build would use instead (same C ABI underneath) is in
// libmesh_adaptor.hpp and INTEGRATION.md.
#pragma once

#include <iosfwd>
#include <string>
#include <utility>
#include <vector>

#include "femshell.h"
#include "mesh_io.hpp"

namespace femshell_host {

// fem-shell.h:42-52 (same names)
struct Parameters {
    std::string in_filename;
    std::string out_filename;
    bool debug = false;
    double nu = 0.3;
    double em = 1.0e6;
    double thickness = 1.0;
    bool isOutfileSet = false;
    // extensions (not in the reference): solver controls that libMesh/PETSc take from
    // equation_systems.parameters / -ksp_* options
    double tol = 1e-12;       // libMesh "linear solver tolerance" default (TOLERANCE^2); also -ksp_rtol
    int max_it = 5000;        // libMesh's "linear solver maximum iterations" default; also -ksp_max_it
    // the reference passes -ksp_type / -pc_type through to PETSc (doc/implementation.tex:68-72).  K is SPD and the
    // library's Krylov method is CG: -ksp_type cg is accepted, anything else is reported and replaced by cg;
    // -pc_type jacobi|bjacobi|pbjacobi|none -> 6x6 block-Jacobi, gamg|amg|ml|hypre|mg -> the multigrid preconditioner
    std::string ksp_type = "cg";
    // default: the multigrid.  The reference's default (PETSc's GMRES + ILU) is a stronger preconditioner than point-block
    // Jacobi, whose iteration count grows with the element count (no convergence at 4M triangles); -pc_type bjacobi opts in
    std::string pc_type = "gamg";
    // shell sections (extension): -sections FILE, lines "tag nu E t" ('#' starts a comment): elements whose tag (Gmsh physical
    // entity, ShellMesh::elem_tag) is listed get that material, all others -nu -e -t.  -section_ids FILE: one integer per
    // element in file order, used in place of the mesh's tags (XDA / XDR meshes carry none).
    std::string sections_file, section_ids_file;
    bool sections_requested() const { return !sections_file.empty() || !section_ids_file.empty(); }
    // structural dynamics (extension): -rho R turns the time loop into Newmark steps of the library (femshell_dynamics_*) with
    // -newmark B G (default 1/4 1/2) and mass-proportional damping -damping A; -dt / -steps: length and number of the steps
    // (the coupled program's own -dt / -steps).  -probe NODE: the node whose history the stand-alone program writes.
    double rho = 0.0; // 0: no dynamics
    double dt = 0.0;
    int steps = 0, probe = -1;
    double newmark_beta = 0.25, newmark_gamma = 0.5, damping = 0.0;
    // (-rho with -gravity and neither -dt nor -steps: the density of the self-weight of a static solve)
    bool dynamics_requested() const { return rho > 0.0 && modes == 0 && !(gravity_set && dt <= 0.0 && steps <= 0); }
    // modal analysis (extension, stand-alone program only): -rho R -modes N [-modes_tol T] [-modes_shift S] computes the N lowest
    // pairs of K x = lambda M x (femshell_modes) instead of a static solve; writes <out>_modes.txt and the mode shapes as point
    // arrays of <out>.vtk.  N in 1 .. 28 (the library's block of N + 4 vectors holds at most 32).
    int modes = 0;
    double modes_tol = 1e-6, modes_shift = 0.0;
    bool modes_requested() const { return modes > 0; }
    // prescribed displacements and support reactions (extension, stand-alone program only; the reference fixes dofs to zero,
    // fem-shell.cpp:90-120).  -prescribed FILE: lines "node u v w tx ty tz" ('#' starts a comment), the values of the dofs the
    // boundary ids fix at that node (femshell_set_prescribed: entries at free dofs are ignored).  The file is read with the
    // command line (read_parameters), the node ids are held against the mesh before any device is touched.  -reactions:
    // writes <out>_reactions.txt -- a line "node rx ry rz mx my mz" (%.15e) per node with a fixed dof, then "sum" and the six
    // column sums over ALL nodes -- and the point arrays reaction_f / reaction_m of <out>.vtk (femshell_reactions).
    std::string prescribed_file;
    std::vector<int32_t> prescribed_nodes; // node of every line of the file
    std::vector<int> prescribed_lines;     // ... and its line number
    std::vector<double> prescribed_values; // ... and its six values
    bool reactions = false;
    // element stress resultants and surface stresses (extension, stand-alone program only; the reference writes displacements, its
    // thesis names the stresses as future work).  -stress: after the static solve writes <out>_stress.txt -- a '#' header, then a
    // line "element Nxx Nyy Nzz Nxy Nyz Nzx Mxx Myy Mzz Mxy Myz Mzx vm_top vm_bottom" (%.15e) per element in the order of the mesh
    // file -- and the cell arrays membrane_force, moment (6 components), von_mises_top, von_mises_bottom of <out>.vtk
    // (femshell_element_resultants).
    bool stress = false;
    // nodal stress recovery and the error indicator (extension, stand-alone program only).  -stress_nodes, with or without -stress:
    // after the static solve writes <out>_stress_nodes.txt -- a '#' header, then a line "node N*(6) M*(6) W fold" (%.15e) per node --
    // and <out>_error.txt -- a '#' header with sum e2, sum eta^2 and the relative error sqrt(sum eta^2 / (sum e2 + sum eta^2)), then a
    // line "element e2 eta2" per element in the order of the mesh file --, adds the point arrays membrane_force_nodes, moment_nodes
    // (6 components) and fold and the cell array error_indicator (eta) to <out>.vtk and prints the relative error
    // (femshell_nodal_resultants).  At folds and section changes the jump of N and M is physical and counts as error: the fold
    // column and the section ids let a reader mask those nodes.
    bool stress_nodes = false;
    bool prescribed_requested() const { return !prescribed_file.empty(); }
    // element loads (extension, stand-alone program only; the reference's loads are the nodal forces of the `_f` file): pressure and
    // traction per element (femshell_set_element_loads).  -pressure P: p = P on every element, along the element's own normal.
    // -element_loads FILE: lines "elem p qx qy qz" ('#' starts a comment), elem the element's index in mesh-file order (the index of
    // <out>_stress.txt); elements not listed get zero.  -gravity gx gy gz (needs -rho): q += rho t g, t the element's own thickness
    // under -sections.  The three add up, and the nodal forces of the `_f` file come on top.  The file is read with the command
    // line; the indices are held against the mesh before any device is touched.  Constant in time under -dt / -steps.
    bool pressure_set = false, gravity_set = false;
    double pressure = 0.0, gravity[3] = {0.0, 0.0, 0.0};
    std::string element_loads_file;
    std::vector<int32_t> element_load_elems; // element of every line of the file
    std::vector<int> element_load_lines;     // ... and its line number
    std::vector<double> element_load_values; // ... and its four values
    bool element_loads_requested() const { return pressure_set || gravity_set || !element_loads_file.empty(); }
    // thermal loads (extension, stand-alone program only; the reference has none): temperatures per element
    // (femshell_set_expansion, femshell_set_thermal).  -alpha A: the expansion coefficient, -section_alpha FILE: lines "tag alpha" for
    // the tags of the -sections file (sections not listed keep A).  -temperature TM: the temperature change of the mid-surface of
    // every element, -temperature_gradient TG: the difference top - bottom of every element, top along the element's own normal.
    // -thermal FILE: lines "elem Tm Tg" with the conventions of -element_loads.  Uniform values and the file add up.  All need
    // -alpha; constant in time under -dt / -steps.
    bool alpha_set = false, temperature_set = false, temperature_gradient_set = false;
    double alpha = 0.0, temperature = 0.0, temperature_gradient = 0.0;
    std::string section_alpha_file, thermal_file;
    std::vector<int32_t> section_alpha_tags; // tag of every line of the -section_alpha file
    std::vector<int> section_alpha_lines;    // ... and its line number
    std::vector<double> section_alpha_values;
    std::vector<int32_t> thermal_elems;      // element of every line of the -thermal file
    std::vector<int> thermal_lines;          // ... and its line number
    std::vector<double> thermal_values;      // ... and its two values
    bool thermal_requested() const { return temperature_set || temperature_gradient_set || !thermal_file.empty(); }
    // elastic supports (extension, stand-alone program only; every support of the reference is rigid): femshell_set_foundation and
    // femshell_set_springs.  -foundation KN and -foundation_shear KT: the moduli (kn, kt) of every element.  -element_foundation
    // FILE: lines "elem kn kt" with the conventions of -element_loads, added on top of the uniform values.  -springs FILE: lines
    // "node kx ky kz krx kry krz", node in mesh-file numbering; nodes not listed get no spring.  All values >= 0.  -support_forces,
    // after the static solve: writes <out>_support.txt -- a line "node fx fy fz mx my mz" (%.15e) per node, the force and moment
    // the elastic supports exert on the shell -- and the point arrays support_f / support_m of <out>.vtk; not with -modes or
    // -dt / -steps.  The files are read with the command line; the indices are held against the mesh before any device is touched.
    bool foundation_set = false, foundation_shear_set = false, support_forces = false;
    double foundation = 0.0, foundation_shear = 0.0;
    std::string element_foundation_file, springs_file;
    std::vector<int32_t> foundation_elems;  // element of every line of the -element_foundation file
    std::vector<int> foundation_lines;      // ... and its line number
    std::vector<double> foundation_values;  // ... and its two values
    std::vector<int32_t> spring_nodes;      // node of every line of the -springs file
    std::vector<int> spring_lines;          // ... and its line number
    std::vector<double> spring_values;      // ... and its six values
    bool foundation_requested() const { return foundation_set || foundation_shear_set || !element_foundation_file.empty(); }
    bool springs_requested() const { return !springs_file.empty(); }
    bool supports_requested() const { return foundation_requested() || springs_requested(); }
    // linear buckling (extension, stand-alone program only; the reference has no stability analysis): -buckling N [-buckling_tol T],
    // after the static solve, computes the N load factors of smallest magnitude of (K + lambda K_G(u)) x = 0 with the prestress of
    // the solution (femshell_buckling); writes <out>_buckling.txt -- a '#' header, then a line "index lambda rho" (%.15e) per mode
    // -- and the shapes as point arrays buckling_<k>_u / buckling_<k>_r of <out>.vtk.  N in 1 .. 28 (the library's block of N + 4
    // vectors holds at most 32).  Not with -modes or -dt / -steps.
    int buckling = 0;
    double buckling_tol = 1e-8;
    bool buckling_requested() const { return buckling > 0; }
    // load cases (extension, stand-alone program only; the reference solves the one load of its `_f` file): -load_cases FILE lists
    // one force file per line (load_cases.hpp), each the whole load of its case; the run calls femshell_solve_cases in place of the
    // single solve and writes <out>_case<k>.vtk (k from 1: the displaced mesh with the point vectors displacement and rotation,
    // every digit) and <out>_cases.txt, a line "k file iterations converged rel_residual" (%.15e) per case.  The list is read with
    // the command line.  Not with another analysis or output of the single solve (-modes, -buckling, -dt / -steps, -prescribed,
    // -reactions, -stress, -stress_nodes, -support_forces) and not with another source of loads (-pressure, -element_loads,
    // -gravity, the thermal flags): a case is its force file and nothing else.  The `_f` file of the mesh is not read.
    std::string load_cases_file;
    std::vector<std::string> load_case_files, load_case_names; // the paths as they are opened, the words of the list
    bool load_cases_requested() const { return !load_cases_file.empty(); }
    // load combinations (extension; with -load_cases only): -combinations FILE2 holds one combination per line, a factor per case
    // of the list (load_cases.hpp read_combinations; read with the command line).  After the cases are solved the run calls
    // femshell_combination_envelope and writes <out>_envelope.txt -- a header, then per element in the order of the mesh file its
    // index, the six envelope values (%.15e) and the six governing combinations counted from 1 -- and <out>_envelope.vtk, the
    // undeformed mesh with six double and six int cell arrays.
    std::string combinations_file;
    std::vector<double> combination_factors; // n_combos x n_cases
    bool combinations_requested() const { return !combinations_file.empty(); }
};

// what femshell_set_element_loads takes: rows (p, qx, qy, qz) of the triangles and of the quadrilaterals
struct ElementLoads {
    std::vector<double> tri_load, quad_load;
};
struct SectionTable;
// -pressure, -element_loads and -gravity added up per element (sections: the table -gravity takes the thicknesses from, or nullptr);
// throws std::runtime_error with file name and line number on an element the mesh does not have or one listed twice
ElementLoads build_element_loads(const Parameters &p, const ShellMesh &mesh, const SectionTable *sections);

// what femshell_set_foundation and femshell_set_springs take: rows (kn, kt) of the triangles and of the quadrilaterals (empty: no
// foundation), the nodes of the -springs file and their six values
struct ElasticSupports {
    std::vector<double> tri_k, quad_k;
    std::vector<int32_t> spring_nodes;
    std::vector<double> spring_values;
};
// -foundation, -foundation_shear and -element_foundation added up per element, the -springs file held against the mesh; throws
// std::runtime_error with file name and line number on an element or a node the mesh does not have or one listed twice
ElasticSupports build_elastic_supports(const Parameters &p, const ShellMesh &mesh);

// what femshell_set_sections takes, from the files above: section 0 is the command line's material, the listed ones follow
struct SectionTable {
    std::vector<femshell_section> sections;
    std::vector<int32_t> tri_section, quad_section;
    std::vector<int32_t> tags; // of section 1 + i, as the -sections file lists them
};
// what femshell_set_expansion and femshell_set_thermal take: rows (Tm, Tg) of the triangles and of the quadrilaterals, and one
// alpha per section under -section_alpha (empty: -alpha for every element)
struct ThermalLoads {
    std::vector<double> tri_temp, quad_temp, section_alpha;
};
// -temperature, -temperature_gradient and -thermal added up per element, -section_alpha held against the table's tags; throws
// std::runtime_error with file name and line number on an element the mesh does not have, one listed twice, a tag the -sections
// file does not list
ThermalLoads build_thermal_loads(const Parameters &p, const ShellMesh &mesh, const SectionTable *sections);
// Reads the files (std::runtime_error with file name and line number on a malformed line), gives every element its section
// and leaves the tags that were used in mesh.elem_tag (the output files show them as the cell array "section").
SectionTable read_sections(const Parameters &p, ShellMesh &mesh);

// One process per GPU.  How a rank learns its place: FEMSHELL_RANK / FEMSHELL_WORLD_SIZE, else the
// launcher's variables (torchrun: RANK / WORLD_SIZE / LOCAL_RANK; Open MPI: OMPI_COMM_WORLD_*; MPICH/Slurm: PMI_RANK /
// PMI_SIZE), else a single rank.  The 128-byte RCCL id travels through a file: rank 0 writes FEMSHELL_UID_FILE
// (default: $XDG_RUNTIME_DIR or /tmp/femshell-<uid>, 0700, file femshell_uid_<MASTER_PORT or parent pid>), the others wait for it -- the role MPI plays for the
// reference (LibMeshInit, fem-shell.cpp:28).
// FEMSHELL_TIMING=1: the wall time of the program's phases, one line on stderr when rank 0 is done (the reference's runs end
// with libMesh's performance log; this is the twin's short form of it)
class PhaseClock {
public:
    PhaseClock();
    void done(const std::string &phase); // closes the phase that ran since the last call (or since construction)
    void note(const std::string &text) { notes_.push_back(text); }
    void report(std::ostream &err) const;

private:
    bool enabled_ = false;
    double start_ = 0.0, last_ = 0.0;
    std::vector<std::pair<std::string, double>> phases_;
    std::vector<std::string> notes_;
};

struct Launch {
    int rank = 0, world_size = 1, device = -1;
    std::string uid_file;
    static Launch from_environment();
};

// Same flags, defaults, messages and return convention as SA:194-267.
bool read_parameters(int argc, char **argv, Parameters &p, std::ostream &out, std::ostream &err);

struct SolveResult {
    unsigned int iterations = 0; // what LinearSolver::solve returns first
    double final_residual = 0.0; // ... and second
    bool converged = false;
    femshell_solve_info info{};
};

class ShellSystem {
  public:
    // throws std::runtime_error on any library error (libMesh code throws / asserts likewise)
    ShellSystem(const Parameters &p, int device = -1, int rank = 0, int world_size = 1, unsigned flags = FEMSHELL_REF_DEFAULT);
    ~ShellSystem();
    ShellSystem(const ShellSystem &) = delete;
    ShellSystem &operator=(const ShellSystem &) = delete;

    // the ShellSystem of this process as the launch environment describes it: context on the rank's GPU, RCCL id
    // exchanged, preconditioner chosen from p.pc_type
    ShellSystem(const Parameters &p, const Launch &launch, unsigned flags = FEMSHELL_REF_DEFAULT);
    void comm_init(const unsigned char id[128]);
    int rank() const { return rank_; }
    // mesh + boundary ids + nodal forces (what main() sets up before init(), SA:35-125)
    void set_mesh(const ShellMesh &m);
    void set_forces(const std::vector<double> &f6); // n_nodes x 6, replaces the `forces` global
    void set_sections(const SectionTable &t);       // after set_mesh (femshell_set_mesh forgets the sections)
    // -prescribed: the file's values (after set_mesh; throws on a node the mesh does not have, with file and line)
    void set_prescribed(const Parameters &p);
    // -pressure / -element_loads / -gravity: the rows of build_element_loads (after set_mesh)
    void set_element_loads(const ElementLoads &l);
    // -alpha / -temperature / -temperature_gradient / -thermal: the rows of build_thermal_loads (after set_mesh and set_sections)
    void set_thermal(const Parameters &p, const ThermalLoads &l);
    // -foundation / -foundation_shear / -element_foundation / -springs: the rows of build_elastic_supports (after set_mesh)
    void set_supports(const ElasticSupports &s);
    // -reactions: r = K_unc u - loads of the last solve's solution, n_nodes x 6
    std::vector<double> reactions();
    // -support_forces: -K_sup u of the last solve's solution, n_nodes x 6
    std::vector<double> support_forces();
    // -stress: the element resultants of the last solve's solution, (n_tri + n_quad) x 14, triangles then quadrilaterals
    std::vector<double> element_resultants();
    // -stress_nodes: the recovered node rows (n_nodes x 14) and the element rows (e2, eta^2; triangles then quadrilaterals) of the
    // last solve's solution
    void nodal_resultants(std::vector<double> &nodes, std::vector<double> &elems);
    // per node: the Dirichlet mask in force (what set_mesh derived from the boundary ids)
    const std::vector<uint8_t> &dirichlet_mask() const { return mask_; }
    // the assembly callback (SA:1160-1233); the name argument is checked like SA:1163
    void assemble_elasticity(const std::string &system_name = "Elasticity");
    // equation_systems.solve(): runs the callback if K is not current, then the Krylov solve
    SolveResult solve(double tol, int max_it);
    // sols[6*node + var] on every rank (SA:141, 163-169)
    const std::vector<double> &build_solution_vector();
    // structural dynamics: density -rho, then Newmark steps of length dt from rest under the loads in force.  dynamics_step
    // computes the candidate of the step (again from the same committed state when it is called twice: a repeated coupling
    // iteration) and leaves its displacements in build_solution_vector(); dynamics_accept commits it.
    void dynamics_begin(const Parameters &p, double dt);
    SolveResult dynamics_step(double tol, int max_it);
    void dynamics_accept();
    // modal analysis: density -rho, then femshell_modes with the library's defaults for guard and iteration limit; lambda[n],
    // modes[n][n_nodes][6], residual[n]
    femshell_modal_info modes(const Parameters &p, std::vector<double> &lambda, std::vector<double> &modes, std::vector<double> &residual);
    // linear buckling under the prestress of the last solve: femshell_buckling with the library's defaults for guard and iteration
    // limit; lambda[n], shapes[n][n_nodes][6], rho[n]
    femshell_buckling_info buckling(const Parameters &p, std::vector<double> &lambda, std::vector<double> &shapes, std::vector<double> &rho);
    // -load_cases: femshell_solve_cases for loads[n_cases][n_nodes][6]; u in the same layout, one info per case
    femshell_cases_info solve_cases(const std::vector<double> &loads, int n_cases, double tol, int max_it, std::vector<double> &u,
                                    std::vector<femshell_case_info> &cases);
    // -combinations: femshell_combination_envelope for u[n_cases][n_nodes][6] and factors[n_combos][n_cases] (no case carries
    // temperatures: -load_cases refuses the thermal options); env and gov hold six values per element, triangles then quadrilaterals
    femshell_envelope_info combination_envelope(const std::vector<double> &u, int n_cases, const std::vector<double> &factors,
                                                std::vector<double> &env, std::vector<int32_t> &gov);
    femshell_ctx *handle() { return ctx_; }

  private:
    void choose_preconditioner(const Parameters &p);
    femshell_ctx *ctx_ = nullptr;
    int n_nodes_ = 0, n_elems_ = 0, rank_ = 0;
    bool solved_once_ = false; // later solves start from the solution before (libMesh's initial guess: ShellSystem::solve)
    std::vector<double> sols_;
    std::vector<uint8_t> mask_;
};

// The stand-alone program (SA:14-185); returns the process exit code.
int fem_shell_main(int argc, char **argv, std::ostream &out, std::ostream &err);

} // namespace femshell_host
