// shell_system.cpp -- see shell_system.hpp
#include "shell_system.hpp"
#include "load_cases.hpp"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <fstream>
#include <sstream>
#include <iostream>
#include <stdexcept>
#include <thread>

#include <fcntl.h>
#include <sys/stat.h>
#include <sys/types.h>
#include <time.h>
#include <unistd.h>

namespace femshell_host {

namespace {

void check(int rc, const char *what)
{
    if (rc != FEMSHELL_OK) throw std::runtime_error(std::string(what) + ": " + femshell_last_error());
}

// GetPot-like lookup: value following `flag`, if present
const char *arg_after(int argc, char **argv, const char *flag)
{
    for (int i = 1; i + 1 < argc; i++)
        if (std::strcmp(argv[i], flag) == 0) return argv[i + 1];
    return nullptr;
}

bool has_flag(int argc, char **argv, const char *flag)
{
    for (int i = 1; i < argc; i++)
        if (std::strcmp(argv[i], flag) == 0) return true;
    return false;
}

} // namespace

// -prescribed FILE into p.prescribed_*: the conventions of the -sections reader ('#' comments, blank lines, file and line number
// in every message)
static void read_prescribed(Parameters &p)
{
    std::ifstream in(p.prescribed_file);
    if (!in) throw std::runtime_error("cannot open " + p.prescribed_file);
    p.prescribed_nodes.clear();
    p.prescribed_lines.clear();
    p.prescribed_values.clear();
    std::string line;
    for (int no = 1; std::getline(in, line); no++) {
        const size_t h = line.find('#');
        if (h != std::string::npos) line.erase(h);
        std::istringstream is(line);
        std::string first;
        if (!(is >> first)) continue; // blank or comment
        const std::string where = p.prescribed_file + ": line " + std::to_string(no) + ": ";
        char *end = nullptr;
        const long node = std::strtol(first.c_str(), &end, 10);
        double v[6];
        std::string rest;
        if (*end != '\0' || !(is >> v[0] >> v[1] >> v[2] >> v[3] >> v[4] >> v[5]) || (is >> rest))
            throw std::runtime_error(where + "expected 'node u v w tx ty tz'");
        for (double x : v)
            if (!std::isfinite(x)) throw std::runtime_error(where + "a value is not finite");
        if (node < 0 || node > 2147483647L) throw std::runtime_error(where + "node id " + first + " is out of range");
        if (std::find(p.prescribed_nodes.begin(), p.prescribed_nodes.end(), (int32_t)node) != p.prescribed_nodes.end())
            throw std::runtime_error(where + "node " + first + " is listed twice");
        p.prescribed_nodes.push_back((int32_t)node);
        p.prescribed_lines.push_back(no);
        p.prescribed_values.insert(p.prescribed_values.end(), v, v + 6);
    }
}

// ... and against the mesh: every listed node must exist
static void check_prescribed_nodes(const Parameters &p, int32_t n_nodes)
{
    for (size_t i = 0; i < p.prescribed_nodes.size(); i++)
        if (p.prescribed_nodes[i] >= n_nodes)
            throw std::runtime_error(p.prescribed_file + ": line " + std::to_string(p.prescribed_lines[i]) + ": node id " +
                                     std::to_string(p.prescribed_nodes[i]) + " is out of range (the mesh has " + std::to_string(n_nodes) + " nodes)");
}

// -element_loads FILE into p.element_load_*: the conventions of the -prescribed reader
static void read_element_loads(Parameters &p)
{
    std::ifstream in(p.element_loads_file);
    if (!in) throw std::runtime_error("cannot open " + p.element_loads_file);
    p.element_load_elems.clear();
    p.element_load_lines.clear();
    p.element_load_values.clear();
    std::string line;
    for (int no = 1; std::getline(in, line); no++) {
        const size_t h = line.find('#');
        if (h != std::string::npos) line.erase(h);
        std::istringstream is(line);
        std::string first;
        if (!(is >> first)) continue; // blank or comment
        const std::string where = p.element_loads_file + ": line " + std::to_string(no) + ": ";
        char *end = nullptr;
        const long elem = std::strtol(first.c_str(), &end, 10);
        double v[4];
        std::string rest;
        if (*end != '\0' || !(is >> v[0] >> v[1] >> v[2] >> v[3]) || (is >> rest)) throw std::runtime_error(where + "expected 'elem p qx qy qz'");
        for (double x : v)
            if (!std::isfinite(x)) throw std::runtime_error(where + "a value is not finite");
        if (elem < 0 || elem > 2147483647L) throw std::runtime_error(where + "element index " + first + " is out of range");
        p.element_load_elems.push_back((int32_t)elem);
        p.element_load_lines.push_back(no);
        p.element_load_values.insert(p.element_load_values.end(), v, v + 4);
    }
}

// -thermal FILE into p.thermal_*: the conventions of the -element_loads reader
static void read_thermal(Parameters &p)
{
    std::ifstream in(p.thermal_file);
    if (!in) throw std::runtime_error("cannot open " + p.thermal_file);
    p.thermal_elems.clear();
    p.thermal_lines.clear();
    p.thermal_values.clear();
    std::string line;
    for (int no = 1; std::getline(in, line); no++) {
        const size_t h = line.find('#');
        if (h != std::string::npos) line.erase(h);
        std::istringstream is(line);
        std::string first;
        if (!(is >> first)) continue; // blank or comment
        const std::string where = p.thermal_file + ": line " + std::to_string(no) + ": ";
        char *end = nullptr;
        const long elem = std::strtol(first.c_str(), &end, 10);
        double v[2];
        std::string rest;
        if (*end != '\0' || !(is >> v[0] >> v[1]) || (is >> rest)) throw std::runtime_error(where + "expected 'elem Tm Tg'");
        for (double x : v)
            if (!std::isfinite(x)) throw std::runtime_error(where + "a value is not finite");
        if (elem < 0 || elem > 2147483647L) throw std::runtime_error(where + "element index " + first + " is out of range");
        p.thermal_elems.push_back((int32_t)elem);
        p.thermal_lines.push_back(no);
        p.thermal_values.insert(p.thermal_values.end(), v, v + 2);
    }
}

// lines 'index v1 .. vN' of stiffnesses (finite, >= 0) into (ids, lines, values): the conventions of the -element_loads reader;
// `expected`: the line's form for the message
static void read_stiffness_rows(const std::string &file, int n_values, const char *expected, std::vector<int32_t> &ids, std::vector<int> &lines,
                                std::vector<double> &values)
{
    std::ifstream in(file);
    if (!in) throw std::runtime_error("cannot open " + file);
    ids.clear();
    lines.clear();
    values.clear();
    std::string line;
    for (int no = 1; std::getline(in, line); no++) {
        const size_t h = line.find('#');
        if (h != std::string::npos) line.erase(h);
        std::istringstream is(line);
        std::string first;
        if (!(is >> first)) continue; // blank or comment
        const std::string where = file + ": line " + std::to_string(no) + ": ";
        char *end = nullptr;
        const long id = std::strtol(first.c_str(), &end, 10);
        double v[6];
        bool ok = *end == '\0';
        for (int k = 0; ok && k < n_values; k++) ok = bool(is >> v[k]);
        std::string rest;
        if (!ok || (is >> rest)) throw std::runtime_error(where + "expected '" + expected + "'");
        for (int k = 0; k < n_values; k++) {
            if (!std::isfinite(v[k])) throw std::runtime_error(where + "a value is not finite");
            if (v[k] < 0.0) throw std::runtime_error(where + "a stiffness is negative");
        }
        if (id < 0 || id > 2147483647L) throw std::runtime_error(where + "index " + first + " is out of range");
        ids.push_back((int32_t)id);
        lines.push_back(no);
        values.insert(values.end(), v, v + n_values);
    }
}

ElasticSupports build_elastic_supports(const Parameters &p, const ShellMesh &mesh)
{
    ElasticSupports s;
    if (p.foundation_requested()) {
        const size_t ne = mesh.order.size();
        std::vector<double> rows(2 * ne, 0.0); // mesh-file order
        std::vector<uint8_t> listed(ne, 0);
        for (size_t i = 0; i < p.foundation_elems.size(); i++) {
            const std::string where = p.element_foundation_file + ": line " + std::to_string(p.foundation_lines[i]) + ": ";
            const size_t e = (size_t)p.foundation_elems[i];
            if (e >= ne)
                throw std::runtime_error(where + "element index " + std::to_string(e) + " is out of range (the mesh has " + std::to_string(ne) + " elements)");
            if (listed[e]) throw std::runtime_error(where + "element " + std::to_string(e) + " is listed twice");
            listed[e] = 1;
            for (int v = 0; v < 2; v++) rows[2 * e + v] = p.foundation_values[2 * i + v];
        }
        s.tri_k.assign(2 * (size_t)mesh.n_tri(), 0.0);
        s.quad_k.assign(2 * (size_t)mesh.n_quad(), 0.0);
        for (size_t e = 0; e < ne; e++) {
            const bool tri = mesh.order[e].first == 't';
            const size_t k = (size_t)mesh.order[e].second;
            double *dst = tri ? &s.tri_k[2 * k] : &s.quad_k[2 * k];
            dst[0] = rows[2 * e] + (p.foundation_set ? p.foundation : 0.0);
            dst[1] = rows[2 * e + 1] + (p.foundation_shear_set ? p.foundation_shear : 0.0);
        }
    }
    std::vector<uint8_t> listed((size_t)mesh.n_nodes(), 0);
    for (size_t i = 0; i < p.spring_nodes.size(); i++) {
        const std::string where = p.springs_file + ": line " + std::to_string(p.spring_lines[i]) + ": ";
        const size_t a = (size_t)p.spring_nodes[i];
        if (a >= (size_t)mesh.n_nodes())
            throw std::runtime_error(where + "node id " + std::to_string(a) + " is out of range (the mesh has " + std::to_string(mesh.n_nodes()) + " nodes)");
        if (listed[a]) throw std::runtime_error(where + "node " + std::to_string(a) + " is listed twice");
        listed[a] = 1;
    }
    s.spring_nodes = p.spring_nodes;
    s.spring_values = p.spring_values;
    return s;
}

// -section_alpha FILE into p.section_alpha_*: lines 'tag alpha'
static void read_section_alpha(Parameters &p)
{
    std::ifstream in(p.section_alpha_file);
    if (!in) throw std::runtime_error("cannot open " + p.section_alpha_file);
    p.section_alpha_tags.clear();
    p.section_alpha_lines.clear();
    p.section_alpha_values.clear();
    std::string line;
    for (int no = 1; std::getline(in, line); no++) {
        const size_t h = line.find('#');
        if (h != std::string::npos) line.erase(h);
        std::istringstream is(line);
        std::string first;
        if (!(is >> first)) continue; // blank or comment
        const std::string where = p.section_alpha_file + ": line " + std::to_string(no) + ": ";
        char *end = nullptr;
        const long tag = std::strtol(first.c_str(), &end, 10);
        double a = 0.0;
        std::string rest;
        if (*end != '\0' || !(is >> a) || (is >> rest)) throw std::runtime_error(where + "expected 'tag alpha'");
        if (!std::isfinite(a)) throw std::runtime_error(where + "a value is not finite");
        if (std::find(p.section_alpha_tags.begin(), p.section_alpha_tags.end(), (int32_t)tag) != p.section_alpha_tags.end())
            throw std::runtime_error(where + "tag " + first + " is listed twice");
        p.section_alpha_tags.push_back((int32_t)tag);
        p.section_alpha_lines.push_back(no);
        p.section_alpha_values.push_back(a);
    }
}

ThermalLoads build_thermal_loads(const Parameters &p, const ShellMesh &mesh, const SectionTable *sections)
{
    const size_t ne = mesh.order.size();
    std::vector<double> rows(2 * ne, 0.0); // mesh-file order
    std::vector<uint8_t> listed(ne, 0);
    for (size_t i = 0; i < p.thermal_elems.size(); i++) {
        const std::string where = p.thermal_file + ": line " + std::to_string(p.thermal_lines[i]) + ": ";
        const size_t e = (size_t)p.thermal_elems[i];
        if (e >= ne)
            throw std::runtime_error(where + "element index " + std::to_string(e) + " is out of range (the mesh has " + std::to_string(ne) + " elements)");
        if (listed[e]) throw std::runtime_error(where + "element " + std::to_string(e) + " is listed twice");
        listed[e] = 1;
        for (int v = 0; v < 2; v++) rows[2 * e + v] = p.thermal_values[2 * i + v];
    }
    ThermalLoads l;
    l.tri_temp.assign(2 * (size_t)mesh.n_tri(), 0.0);
    l.quad_temp.assign(2 * (size_t)mesh.n_quad(), 0.0);
    for (size_t e = 0; e < ne; e++) {
        const bool tri = mesh.order[e].first == 't';
        const size_t k = (size_t)mesh.order[e].second;
        double *dst = tri ? &l.tri_temp[2 * k] : &l.quad_temp[2 * k];
        dst[0] = rows[2 * e] + (p.temperature_set ? p.temperature : 0.0);
        dst[1] = rows[2 * e + 1] + (p.temperature_gradient_set ? p.temperature_gradient : 0.0);
    }
    if (!p.section_alpha_file.empty()) {
        if (!sections) throw std::runtime_error(p.section_alpha_file + ": -section_alpha needs the sections of a -sections file");
        l.section_alpha.assign(sections->sections.size(), p.alpha);
        for (size_t i = 0; i < p.section_alpha_tags.size(); i++) {
            const auto it = std::find(sections->tags.begin(), sections->tags.end(), p.section_alpha_tags[i]);
            if (it == sections->tags.end())
                throw std::runtime_error(p.section_alpha_file + ": line " + std::to_string(p.section_alpha_lines[i]) + ": tag " +
                                         std::to_string(p.section_alpha_tags[i]) + " is not a tag of the -sections file");
            l.section_alpha[(size_t)(it - sections->tags.begin()) + 1] = p.section_alpha_values[i];
        }
    }
    return l;
}

ElementLoads build_element_loads(const Parameters &p, const ShellMesh &mesh, const SectionTable *sections)
{
    const size_t ne = mesh.order.size();
    std::vector<double> rows(4 * ne, 0.0); // mesh-file order
    std::vector<uint8_t> listed(ne, 0);
    for (size_t i = 0; i < p.element_load_elems.size(); i++) {
        const std::string where = p.element_loads_file + ": line " + std::to_string(p.element_load_lines[i]) + ": ";
        const size_t e = (size_t)p.element_load_elems[i];
        if (e >= ne)
            throw std::runtime_error(where + "element index " + std::to_string(e) + " is out of range (the mesh has " + std::to_string(ne) + " elements)");
        if (listed[e]) throw std::runtime_error(where + "element " + std::to_string(e) + " is listed twice");
        listed[e] = 1;
        for (int v = 0; v < 4; v++) rows[4 * e + v] = p.element_load_values[4 * i + v];
    }
    ElementLoads l;
    l.tri_load.assign(4 * (size_t)mesh.n_tri(), 0.0);
    l.quad_load.assign(4 * (size_t)mesh.n_quad(), 0.0);
    for (size_t e = 0; e < ne; e++) {
        const bool tri = mesh.order[e].first == 't';
        const size_t k = (size_t)mesh.order[e].second;
        double *dst = tri ? &l.tri_load[4 * k] : &l.quad_load[4 * k];
        for (int v = 0; v < 4; v++) dst[v] = rows[4 * e + v];
        if (p.pressure_set) dst[0] += p.pressure;
        if (p.gravity_set) {
            const double t = sections ? sections->sections[(size_t)(tri ? sections->tri_section : sections->quad_section)[k]].thickness : p.thickness;
            for (int d = 0; d < 3; d++) dst[1 + d] += p.rho * t * p.gravity[d];
        }
    }
    return l;
}

bool read_parameters(int argc, char **argv, Parameters &p, std::ostream &out, std::ostream &err)
{
    if (argc < 5) {
        err << "Error, must choose valid parameters.\n"
            << "Usage: " << argv[0] << " -nu -e -t -mesh [-out] [-d]\n"
            << "-nu:\t Possion's ratio (required)\n"
            << "-e:\t Elastic/Young's modulus E (required)\n"
            << "-t:\t Thickness (required)\n"
            << "-mesh:\t Input mesh file (*.xda, required)\n"
            << "-out:\t Output file name (without extension, optional)\n"
            << "-d:\t Additional (debug) messages (1=on, 0=off (default))\n"
            << "-tol:\t relative residual tolerance of the CG solve (optional, default 1e-12)\n"
            << "-max_it:\t iteration limit of the CG solve (optional, default 5000)\n"
            << "-pc_type:\t gamg (multigrid, default) | bjacobi (6x6 block-Jacobi)\n"
            << "-sections:\t file of lines 'tag nu E t': material of the elements with that tag (optional; others: -nu -e -t)\n"
            << "-section_ids:\t file with one tag per element, in place of the mesh file's tags (optional)\n"
            << "-rho:\t mass density: structural dynamics, -steps Newmark steps of length -dt under the force file's loads as a\n"
            << "\t step load at t = 0; writes <out>_history.txt, lines 't u v w' of the probe node (optional)\n"
            << "-dt:\t time step length (with -rho)\n"
            << "-steps:\t number of time steps (with -rho)\n"
            << "-probe:\t node of the history (optional, default: the node of largest load)\n"
            << "-newmark:\t beta gamma of Newmark's method (optional, default 0.25 0.5)\n"
            << "-damping:\t mass-proportional damping C = A M (optional, default 0)\n"
            << "-modes:\t with -rho: the N lowest natural frequencies and mode shapes instead of a solve (N in 1 .. 28); writes\n"
            << "\t <out>_modes.txt, lines 'index lambda f residual', and the shapes as point arrays mode_<k>_u / mode_<k>_r of <out>.vtk\n"
            << "-modes_tol:\t tolerance of the pairs' residuals (with -modes, default 1e-6)\n"
            << "-modes_shift:\t shift S >= 0: solves with K + S M (with -modes; an unconstrained shell needs S > 0; default 0)\n"
            << "-prescribed:\t file of lines 'node u v w tx ty tz': prescribed displacements of the dofs the boundary ids fix (optional)\n"
            << "-reactions:\t writes <out>_reactions.txt, lines 'node rx ry rz mx my mz' of the nodes with a fixed dof and a line 'sum',\n"
            << "\t and the point arrays reaction_f / reaction_m of <out>.vtk (optional)\n"
            << "-stress:\t writes <out>_stress.txt, a line per element with the membrane force tensor N, the moment tensor M (global axes,\n"
            << "\t xx yy zz xy yz zx) and the von Mises stress at the top and the bottom surface (element means), and the cell arrays\n"
            << "\t membrane_force, moment, von_mises_top, von_mises_bottom of <out>.vtk (optional)\n"
            << "-stress_nodes:\t writes <out>_stress_nodes.txt, a line per node with the element tensors averaged to the node (N*, M*), the\n"
            << "\t area W it was averaged over and the fold measure, and <out>_error.txt, the Zienkiewicz-Zhu indicator (e2, eta2) per\n"
            << "\t element under a header with the sums and the relative error of the mesh; point arrays membrane_force_nodes,\n"
            << "\t moment_nodes, fold and the cell array error_indicator of <out>.vtk (optional; with or without -stress; jumps at\n"
            << "\t folds and section changes count as error)\n"
            << "-pressure:\t uniform pressure P on every element, along the element's own normal (optional; dead load, lumped to the nodes)\n"
            << "-element_loads:\t file of lines 'elem p qx qy qz': pressure and traction per area (global axes) of the element with that index\n"
            << "\t in mesh-file order, the index of <out>_stress.txt; elements not listed get zero (optional)\n"
            << "-gravity:\t gx gy gz: self-weight rho t g per area of every element, t the element's own under -sections (needs -rho; without\n"
            << "\t -dt / -steps the solve stays static)\n"
            << "\t -pressure, -element_loads and -gravity add up and come on top of the force file's nodal loads; not with -modes\n"
            << "-alpha:\t thermal expansion coefficient A (needed by the temperature options below)\n"
            << "-section_alpha:\t file of lines 'tag alpha': expansion coefficient of the sections with that tag of the -sections file\n"
            << "\t (optional; sections not listed keep -alpha)\n"
            << "-temperature:\t temperature change TM of the mid-surface of every element (optional)\n"
            << "-temperature_gradient:\t temperature difference TG = top - bottom of every element, top along the element's own normal\n"
            << "-thermal:\t file of lines 'elem Tm Tg': temperatures of the element with that index in mesh-file order (optional)\n"
            << "\t -temperature, -temperature_gradient and -thermal add up; the work-equivalent loads come on top of all other loads, and\n"
            << "\t -stress, -reactions and -buckling work on the heated shell; not with -modes\n"
            << "-foundation:\t elastic foundation modulus KN >= 0 of every element along its own normal, force per volume (optional)\n"
            << "-foundation_shear:\t ... and KT >= 0 in the element's plane (optional)\n"
            << "-element_foundation:\t file of lines 'elem kn kt': moduli of the element with that index in mesh-file order, added on top of\n"
            << "\t the uniform values (optional)\n"
            << "-springs:\t file of lines 'node kx ky kz krx kry krz': springs >= 0 in global axes at the node with that id (optional)\n"
            << "\t the supports are part of K: the solve, -dt / -steps, -modes, -buckling, -reactions and -stress see the supported shell\n"
            << "-support_forces:\t after the static solve: writes <out>_support.txt, lines 'node fx fy fz mx my mz', the force and moment the\n"
            << "\t elastic supports exert on the shell, and the point arrays support_f / support_m of <out>.vtk (optional; not with\n"
            << "\t -modes or -dt / -steps)\n"
            << "-buckling:\t after the static solve: the N load factors of smallest magnitude (signed) at which the solved load case\n"
            << "\t buckles, N in 1 .. 28; writes <out>_buckling.txt, lines 'index lambda rho', and the shapes as point arrays\n"
            << "\t buckling_<k>_u / buckling_<k>_r of <out>.vtk (optional; not with -modes or -dt / -steps)\n"
            << "-buckling_tol:\t tolerance of the pairs' convergence measure rho (with -buckling, default 1e-8)\n"
            << "-load_cases:\t file that lists one force file per line (at most 32; '#' comments; paths relative to the list): every file\n"
            << "\t is the whole load of one case on the same model, all solved in one call in place of the single solve; writes\n"
            << "\t <out>_case<k>.vtk and <out>_cases.txt, lines 'k file iterations converged rel_residual' (optional; the mesh's own\n"
            << "\t force file is not read; not with -modes, -buckling, -dt / -steps, -prescribed, -reactions, -stress, -stress_nodes,\n"
            << "\t -support_forces, nor with -pressure, -element_loads, -gravity or the thermal options)\n"
            << "-combinations:\t with -load_cases: file with one load combination per line, a factor per listed case (at most 256 lines;\n"
            << "\t '#' comments); writes <out>_envelope.txt, per element the largest surface von Mises stresses, the extreme principal\n"
            << "\t membrane forces and moments over all combinations and the combination (from 1) that governs each, and the same as\n"
            << "\t cell arrays of <out>_envelope.vtk (optional)\n";
        return false;
    }
    bool failed = false;
    if (const char *v = arg_after(argc, argv, "-d")) p.debug = std::atoi(v) == 1;
    if (has_flag(argc, argv, "-nu")) {
        const char *v = arg_after(argc, argv, "-nu");
        p.nu = v ? std::atof(v) : 0.3;
    } else {
        err << "ERROR: Poisson's ratio nu not specified!\n";
        failed = true;
    }
    if (has_flag(argc, argv, "-e")) {
        const char *v = arg_after(argc, argv, "-e");
        p.em = v ? std::atof(v) : 1.0e6;
    } else {
        err << "ERROR: Elastic modulus E not specified!\n";
        failed = true;
    }
    if (has_flag(argc, argv, "-t")) {
        const char *v = arg_after(argc, argv, "-t");
        p.thickness = v ? std::atof(v) : 1.0;
    } else {
        err << "ERROR: Mesh thickness t not specified!\n";
        failed = true;
    }
    if (has_flag(argc, argv, "-mesh")) {
        const char *v = arg_after(argc, argv, "-mesh");
        p.in_filename = v ? v : "mesh.xda";
    } else {
        err << "ERROR: Mesh file not specified!\n";
        failed = true;
    }
    if (has_flag(argc, argv, "-out")) {
        const char *v = arg_after(argc, argv, "-out");
        p.out_filename = v ? v : "out";
        p.isOutfileSet = true;
    } else {
        p.isOutfileSet = false;
    }
    if (const char *v = arg_after(argc, argv, "-sections")) p.sections_file = v;
    if (const char *v = arg_after(argc, argv, "-section_ids")) p.section_ids_file = v;
    if (const char *v = arg_after(argc, argv, "-tol")) p.tol = std::atof(v);
    if (const char *v = arg_after(argc, argv, "-max_it")) p.max_it = std::atoi(v);
    // PETSc-style options the reference's users pass on the same command line (doc/implementation.tex:68-72)
    if (const char *v = arg_after(argc, argv, "-ksp_rtol")) p.tol = std::atof(v);
    if (const char *v = arg_after(argc, argv, "-ksp_max_it")) p.max_it = std::atoi(v);
    if (const char *v = arg_after(argc, argv, "-ksp_type")) {
        p.ksp_type = v;
        if (p.ksp_type != "cg") {
            err << "NOTE: -ksp_type " << p.ksp_type << " is not available: K is symmetric positive definite and the solve on the GPU"
                << " is a conjugate-gradient method; using -ksp_type cg\n";
            p.ksp_type = "cg";
        }
    }
    if (const char *v = arg_after(argc, argv, "-pc_type")) {
        p.pc_type = v;
        static const char *known[] = {"jacobi", "bjacobi", "pbjacobi", "gamg", "amg", "ml", "hypre", "mg"};
        bool ok = false;
        for (const char *k : known) ok = ok || p.pc_type == k;
        if (p.pc_type == "none" || p.pc_type == "ilu" || p.pc_type == "icc" || p.pc_type == "sor" || p.pc_type == "asm" || p.pc_type == "lu") {
            // PETSc's own defaults (ilu serial, bjacobi + ilu parallel) and other host-side preconditioners: handled like an
            // unavailable -ksp_type -- say what runs instead, do not fail
            err << "NOTE: -pc_type " << p.pc_type << " is not available on the GPU; using the 6x6 block-Jacobi preconditioner"
                << " (-pc_type gamg selects the multigrid)\n";
            p.pc_type = "pbjacobi";
        } else if (!ok) {
            err << "ERROR: -pc_type " << p.pc_type << " is not available (jacobi|bjacobi|pbjacobi -> 6x6 block-Jacobi, gamg|amg|ml|hypre|mg -> multigrid)\n";
            failed = true;
        }
    }
    // structural dynamics: everything that can be refused is refused here, before any device is touched
    if (has_flag(argc, argv, "-rho")) {
        const char *v = arg_after(argc, argv, "-rho");
        p.rho = v ? std::atof(v) : 0.0;
        if (!(std::isfinite(p.rho) && p.rho > 0.0)) {
            err << "ERROR: -rho must be a density > 0!\n";
            failed = true;
        }
    }
    if (has_flag(argc, argv, "-dt")) {
        const char *v = arg_after(argc, argv, "-dt");
        p.dt = v ? std::atof(v) : 0.0;
        if (!(std::isfinite(p.dt) && p.dt > 0.0)) {
            err << "ERROR: -dt must be a time step length > 0!\n";
            failed = true;
        }
    }
    if (has_flag(argc, argv, "-steps")) {
        const char *v = arg_after(argc, argv, "-steps");
        p.steps = v ? std::atoi(v) : 0;
        if (!has_flag(argc, argv, "-dt")) {
            err << "ERROR: -steps needs a time step length, -dt!\n";
            failed = true;
        }
    }
    if (const char *v = arg_after(argc, argv, "-probe")) p.probe = std::atoi(v);
    if (has_flag(argc, argv, "-newmark")) {
        const char *b = nullptr, *g = nullptr;
        for (int i = 1; i + 2 < argc; i++)
            if (std::strcmp(argv[i], "-newmark") == 0) {
                b = argv[i + 1];
                g = argv[i + 2];
            }
        p.newmark_beta = b ? std::atof(b) : 0.0;
        p.newmark_gamma = g ? std::atof(g) : 0.0;
        // (the unconditionally stable schemes; the limit itself as written in decimals, e.g. 0.3025 0.6)
        if (!(p.newmark_gamma >= 0.5) || !(p.newmark_beta * (1.0 + 1e-12) >= 0.25 * (p.newmark_gamma + 0.5) * (p.newmark_gamma + 0.5))) {
            err << "ERROR: -newmark beta gamma needs gamma >= 1/2 and beta >= (gamma + 1/2)^2 / 4!\n";
            failed = true;
        }
    }
    if (has_flag(argc, argv, "-damping")) {
        const char *v = arg_after(argc, argv, "-damping");
        p.damping = v ? std::atof(v) : -1.0;
        if (!(std::isfinite(p.damping) && p.damping >= 0.0)) {
            err << "ERROR: -damping must be >= 0!\n";
            failed = true;
        }
    }
    // modal analysis: refused here like the dynamics options
    if (has_flag(argc, argv, "-modes")) {
        const char *v = arg_after(argc, argv, "-modes");
        p.modes = v ? std::atoi(v) : 0;
        if (p.modes < 1 || p.modes > 28) {
            err << "ERROR: -modes must be a number of modes in 1 .. 28!\n";
            p.modes = 0;
            failed = true;
        }
        if (!has_flag(argc, argv, "-rho")) {
            err << "ERROR: -modes needs a density, -rho!\n";
            failed = true;
        }
        if (has_flag(argc, argv, "-dt") || has_flag(argc, argv, "-steps")) {
            err << "ERROR: -modes does not go together with the time stepping options -dt / -steps!\n";
            failed = true;
        }
    } else if (has_flag(argc, argv, "-modes_tol") || has_flag(argc, argv, "-modes_shift")) {
        err << "ERROR: -modes_tol / -modes_shift need a number of modes, -modes!\n";
        failed = true;
    }
    if (has_flag(argc, argv, "-modes_tol")) {
        const char *v = arg_after(argc, argv, "-modes_tol");
        p.modes_tol = v ? std::atof(v) : 0.0;
        if (!(std::isfinite(p.modes_tol) && p.modes_tol > 0.0)) {
            err << "ERROR: -modes_tol must be a tolerance > 0!\n";
            failed = true;
        }
    }
    if (has_flag(argc, argv, "-modes_shift")) {
        const char *v = arg_after(argc, argv, "-modes_shift");
        p.modes_shift = v ? std::atof(v) : -1.0;
        if (!(std::isfinite(p.modes_shift) && p.modes_shift >= 0.0)) {
            err << "ERROR: -modes_shift must be a shift >= 0!\n";
            failed = true;
        }
    }
    // linear buckling: refused here like the options above
    if (has_flag(argc, argv, "-buckling")) {
        const char *v = arg_after(argc, argv, "-buckling");
        p.buckling = v ? std::atoi(v) : 0;
        if (p.buckling < 1 || p.buckling > 28) {
            err << "ERROR: -buckling must be a number of load factors in 1 .. 28!\n";
            p.buckling = 0;
            failed = true;
        }
        if (has_flag(argc, argv, "-modes")) {
            err << "ERROR: -buckling follows the static solve: it does not go together with -modes!\n";
            failed = true;
        }
        if (has_flag(argc, argv, "-dt") || has_flag(argc, argv, "-steps")) {
            err << "ERROR: -buckling follows the static solve: it does not go together with the time stepping options -dt / -steps!\n";
            failed = true;
        }
    } else if (has_flag(argc, argv, "-buckling_tol")) {
        err << "ERROR: -buckling_tol needs a number of load factors, -buckling!\n";
        failed = true;
    }
    if (has_flag(argc, argv, "-buckling_tol")) {
        const char *v = arg_after(argc, argv, "-buckling_tol");
        p.buckling_tol = v ? std::atof(v) : 0.0;
        if (!(std::isfinite(p.buckling_tol) && p.buckling_tol > 0.0)) {
            err << "ERROR: -buckling_tol must be a tolerance > 0!\n";
            failed = true;
        }
    }
    // prescribed displacements and reactions: the file is read here, so that a missing file or a malformed line is refused
    // like any other option (the node ids are held against the mesh as soon as it is read, still before any device is touched)
    if (has_flag(argc, argv, "-prescribed")) {
        const char *v = arg_after(argc, argv, "-prescribed");
        p.prescribed_file = v ? v : "";
        if (!v) {
            err << "ERROR: -prescribed needs a file!\n";
            failed = true;
        } else {
            try {
                read_prescribed(p);
            } catch (const std::exception &e) {
                err << "ERROR: " << e.what() << "\n";
                failed = true;
            }
        }
        if (has_flag(argc, argv, "-modes") || has_flag(argc, argv, "-dt") || has_flag(argc, argv, "-steps")) {
            err << "ERROR: -prescribed does not go together with -modes or the time stepping options -dt / -steps!\n";
            failed = true;
        }
    }
    if (has_flag(argc, argv, "-reactions")) {
        p.reactions = true;
        if (has_flag(argc, argv, "-modes") || has_flag(argc, argv, "-dt") || has_flag(argc, argv, "-steps")) {
            err << "ERROR: -reactions belongs to the static solve: not with -modes or the time stepping options -dt / -steps!\n";
            failed = true;
        }
    }
    if (has_flag(argc, argv, "-stress")) {
        p.stress = true;
        if (has_flag(argc, argv, "-modes") || has_flag(argc, argv, "-dt") || has_flag(argc, argv, "-steps")) {
            err << "ERROR: -stress belongs to the static solve: not with -modes or the time stepping options -dt / -steps!\n";
            failed = true;
        }
    }
    if (has_flag(argc, argv, "-stress_nodes")) {
        p.stress_nodes = true;
        if (has_flag(argc, argv, "-modes") || has_flag(argc, argv, "-dt") || has_flag(argc, argv, "-steps")) {
            err << "ERROR: -stress_nodes belongs to the static solve: not with -modes or the time stepping options -dt / -steps!\n";
            failed = true;
        }
    }
    // element loads: refused here like the options above (the element indices are held against the mesh as soon as it is read)
    auto number = [](const char *text, double *value) {
        if (!text) return false;
        char *end = nullptr;
        *value = std::strtod(text, &end);
        return end != text && *end == '\0' && std::isfinite(*value);
    };
    if (has_flag(argc, argv, "-pressure")) {
        p.pressure_set = true;
        if (!number(arg_after(argc, argv, "-pressure"), &p.pressure)) {
            err << "ERROR: -pressure needs a finite number!\n";
            failed = true;
        }
    }
    if (has_flag(argc, argv, "-element_loads")) {
        const char *v = arg_after(argc, argv, "-element_loads");
        p.element_loads_file = v ? v : "";
        if (!v) {
            err << "ERROR: -element_loads needs a file!\n";
            failed = true;
        } else {
            try {
                read_element_loads(p);
            } catch (const std::exception &e) {
                err << "ERROR: " << e.what() << "\n";
                failed = true;
            }
        }
    }
    if (has_flag(argc, argv, "-gravity")) {
        p.gravity_set = true;
        bool ok = false;
        for (int i = 1; i + 3 < argc; i++)
            if (std::strcmp(argv[i], "-gravity") == 0)
                ok = number(argv[i + 1], &p.gravity[0]) && number(argv[i + 2], &p.gravity[1]) && number(argv[i + 3], &p.gravity[2]);
        if (!ok) {
            err << "ERROR: -gravity needs three finite numbers gx gy gz!\n";
            failed = true;
        }
        if (!has_flag(argc, argv, "-rho")) {
            err << "ERROR: -gravity needs a density, -rho!\n";
            failed = true;
        }
    }
    // thermal loads: refused here in the same way
    if (has_flag(argc, argv, "-alpha")) {
        p.alpha_set = true;
        if (!number(arg_after(argc, argv, "-alpha"), &p.alpha)) {
            err << "ERROR: -alpha needs a finite number!\n";
            failed = true;
        }
    }
    if (has_flag(argc, argv, "-temperature")) {
        p.temperature_set = true;
        if (!number(arg_after(argc, argv, "-temperature"), &p.temperature)) {
            err << "ERROR: -temperature needs a finite number!\n";
            failed = true;
        }
    }
    if (has_flag(argc, argv, "-temperature_gradient")) {
        p.temperature_gradient_set = true;
        if (!number(arg_after(argc, argv, "-temperature_gradient"), &p.temperature_gradient)) {
            err << "ERROR: -temperature_gradient needs a finite number!\n";
            failed = true;
        }
    }
    if (has_flag(argc, argv, "-thermal")) {
        const char *v = arg_after(argc, argv, "-thermal");
        p.thermal_file = v ? v : "";
        if (!v) {
            err << "ERROR: -thermal needs a file!\n";
            failed = true;
        } else {
            try {
                read_thermal(p);
            } catch (const std::exception &e) {
                err << "ERROR: " << e.what() << "\n";
                failed = true;
            }
        }
    }
    if (has_flag(argc, argv, "-section_alpha")) {
        const char *v = arg_after(argc, argv, "-section_alpha");
        p.section_alpha_file = v ? v : "";
        if (!v) {
            err << "ERROR: -section_alpha needs a file!\n";
            failed = true;
        } else {
            try {
                read_section_alpha(p);
            } catch (const std::exception &e) {
                err << "ERROR: " << e.what() << "\n";
                failed = true;
            }
        }
        if (!has_flag(argc, argv, "-sections")) {
            err << "ERROR: -section_alpha needs the sections of a -sections file!\n";
            failed = true;
        }
    }
    if ((p.thermal_requested() || has_flag(argc, argv, "-section_alpha")) && !has_flag(argc, argv, "-alpha")) {
        err << "ERROR: -temperature / -temperature_gradient / -thermal / -section_alpha need an expansion coefficient, -alpha!\n";
        failed = true;
    }
    if ((p.thermal_requested() || p.alpha_set || has_flag(argc, argv, "-section_alpha")) && has_flag(argc, argv, "-modes")) {
        err << "ERROR: -alpha / -section_alpha / -temperature / -temperature_gradient / -thermal do not go together with -modes (a modal analysis has no loads)!\n";
        failed = true;
    }
    // elastic supports: refused here in the same way
    if (has_flag(argc, argv, "-foundation")) {
        p.foundation_set = true;
        if (!number(arg_after(argc, argv, "-foundation"), &p.foundation) || p.foundation < 0.0) {
            err << "ERROR: -foundation needs a finite number >= 0!\n";
            failed = true;
        }
    }
    if (has_flag(argc, argv, "-foundation_shear")) {
        p.foundation_shear_set = true;
        if (!number(arg_after(argc, argv, "-foundation_shear"), &p.foundation_shear) || p.foundation_shear < 0.0) {
            err << "ERROR: -foundation_shear needs a finite number >= 0!\n";
            failed = true;
        }
    }
    if (has_flag(argc, argv, "-element_foundation")) {
        const char *v = arg_after(argc, argv, "-element_foundation");
        p.element_foundation_file = v ? v : "";
        if (!v) {
            err << "ERROR: -element_foundation needs a file!\n";
            failed = true;
        } else {
            try {
                read_stiffness_rows(p.element_foundation_file, 2, "elem kn kt", p.foundation_elems, p.foundation_lines, p.foundation_values);
            } catch (const std::exception &e) {
                err << "ERROR: " << e.what() << "\n";
                failed = true;
            }
        }
    }
    if (has_flag(argc, argv, "-springs")) {
        const char *v = arg_after(argc, argv, "-springs");
        p.springs_file = v ? v : "";
        if (!v) {
            err << "ERROR: -springs needs a file!\n";
            failed = true;
        } else {
            try {
                read_stiffness_rows(p.springs_file, 6, "node kx ky kz krx kry krz", p.spring_nodes, p.spring_lines, p.spring_values);
            } catch (const std::exception &e) {
                err << "ERROR: " << e.what() << "\n";
                failed = true;
            }
        }
    }
    if (has_flag(argc, argv, "-support_forces")) {
        p.support_forces = true;
        if (has_flag(argc, argv, "-modes") || has_flag(argc, argv, "-dt") || has_flag(argc, argv, "-steps")) {
            err << "ERROR: -support_forces belongs to the static solve: not with -modes or the time stepping options -dt / -steps!\n";
            failed = true;
        }
    }
    // load cases: the list is read here, so that a missing list, a missing listed file, an empty or too long list and an option
    // that does not go together with it are refused like any other option
    if (has_flag(argc, argv, "-load_cases")) {
        const char *v = arg_after(argc, argv, "-load_cases");
        p.load_cases_file = v ? v : "";
        if (!v) {
            err << "ERROR: -load_cases needs a file!\n";
            failed = true;
        } else {
            try {
                p.load_case_files = read_load_cases_list(p.load_cases_file, &p.load_case_names);
            } catch (const std::exception &e) {
                err << "ERROR: " << e.what() << "\n";
                failed = true;
            }
        }
        const std::string conflicts = load_cases_conflicts(argc, argv);
        if (!conflicts.empty()) {
            err << "ERROR: -load_cases does not go together with " << conflicts
                << ": a case is its force file and nothing else, solved in place of the single static solve!\n";
            failed = true;
        }
    }
    // load combinations: the factors are read here too, against the count of cases the list gave
    if (has_flag(argc, argv, "-combinations")) {
        const char *v = arg_after(argc, argv, "-combinations");
        p.combinations_file = v ? v : "";
        if (!v) {
            err << "ERROR: -combinations needs a file!\n";
            failed = true;
        } else if (!has_flag(argc, argv, "-load_cases")) {
            err << "ERROR: -combinations needs -load_cases: a combination is a row of factors, one per listed load case!\n";
            failed = true;
        } else if (!p.load_case_files.empty()) { // (a refused list has said so already)
            try {
                p.combination_factors = read_combinations(p.combinations_file, (int)p.load_case_files.size());
            } catch (const std::exception &e) {
                err << "ERROR: " << e.what() << "\n";
                failed = true;
            }
        }
    }
    if (p.element_loads_requested() && has_flag(argc, argv, "-modes")) {
        err << "ERROR: -pressure / -element_loads / -gravity do not go together with -modes (a modal analysis has no loads)!\n";
        failed = true;
    }

    out << "Run program with parameters:"
        << " debug messages = " << (p.debug ? "true" : "false") << ", nu = " << p.nu << ", E = " << p.em
        << ", t = " << p.thickness << ", mesh file = " << p.in_filename;
    if (p.isOutfileSet) out << ", out-file = " << p.out_filename;
    out << std::endl;
    return !failed;
}

ShellSystem::ShellSystem(const Parameters &p, int device, int rank, int world_size, unsigned flags)
{
    femshell_config cfg{};
    cfg.nu = p.nu;
    cfg.E = p.em;
    cfg.thickness = p.thickness;
    cfg.flags = flags;
    cfg.device = device;
    cfg.rank = rank;
    cfg.world_size = world_size;
    rank_ = rank;
    check(femshell_create(&cfg, &ctx_), "femshell_create");
}

Launch Launch::from_environment()
{
    auto env_int = [](std::initializer_list<const char *> names, int fallback) {
        for (const char *n : names)
            if (const char *v = std::getenv(n)) return std::atoi(v);
        return fallback;
    };
    Launch l;
    l.rank = env_int({"FEMSHELL_RANK", "RANK", "OMPI_COMM_WORLD_RANK", "PMI_RANK"}, 0);
    l.world_size = env_int({"FEMSHELL_WORLD_SIZE", "WORLD_SIZE", "OMPI_COMM_WORLD_SIZE", "PMI_SIZE"}, 1);
    l.device = env_int({"FEMSHELL_DEVICE", "LOCAL_RANK", "OMPI_COMM_WORLD_LOCAL_RANK"}, -1);
    if (std::getenv("FEMSHELL_SINGLE") && std::atoi(std::getenv("FEMSHELL_SINGLE")) == 1) { // ignore a launcher's RANK / WORLD_SIZE
        l.rank = 0;
        l.world_size = 1;
    }
    if (const char *f = std::getenv("FEMSHELL_UID_FILE")) l.uid_file = f;
    else {
        // per-user directory, not a name in /tmp anyone can squat: $XDG_RUNTIME_DIR, else /tmp/femshell-<uid> (0700, ours)
        std::string dir;
        if (const char *x = std::getenv("XDG_RUNTIME_DIR")) dir = x;
        if (dir.empty()) {
            dir = "/tmp/femshell-" + std::to_string((long)getuid());
            (void)mkdir(dir.c_str(), 0700);
            struct stat st;
            if (lstat(dir.c_str(), &st) != 0 || !S_ISDIR(st.st_mode) || st.st_uid != getuid() || (st.st_mode & 077) != 0)
                throw std::runtime_error("launch environment: " + dir + " is not a private directory of this user (set FEMSHELL_UID_FILE)");
        }
        const char *port = std::getenv("MASTER_PORT");
        l.uid_file = dir + "/femshell_uid_" + (port ? std::string(port) : std::to_string((long)getppid()));
    }
    if (l.world_size < 1 || l.rank < 0 || l.rank >= l.world_size) throw std::runtime_error("launch environment: invalid rank / world size");
    if (l.world_size > 1) // a launcher's generic RANK / WORLD_SIZE turn a plain run into rank k of N: say so
        std::cerr << "fem-shell: rank " << l.rank << " of " << l.world_size << " (from the launch environment; RCCL id through " << l.uid_file
                  << "; FEMSHELL_SINGLE=1 runs single-process regardless)" << std::endl;
    return l;
}

namespace {

// The RCCL id travels through a file: 8 bytes of magic, then the 128-byte id.  Rank 0 removes whatever an earlier run
// left under the name, writes a temporary created with O_EXCL | O_NOFOLLOW and renames it into place; the others accept
// only a regular file of this user that is not older than a minute before their own start (a crashed run's leftover).
constexpr char kUidMagic[8] = {'F', 'S', 'H', 'L', 'U', 'I', 'D', '1'};

void publish_uid(const std::string &path, const unsigned char id[128])
{
    (void)unlink(path.c_str());
    const std::string tmp = path + ".tmp." + std::to_string((long)getpid());
    (void)unlink(tmp.c_str());
    const int fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_EXCL | O_NOFOLLOW | O_CLOEXEC, 0600);
    if (fd < 0) throw std::runtime_error("cannot create " + tmp);
    const bool ok = write(fd, kUidMagic, 8) == 8 && write(fd, id, 128) == 128;
    (void)close(fd);
    if (!ok || std::rename(tmp.c_str(), path.c_str()) != 0) {
        (void)unlink(tmp.c_str());
        throw std::runtime_error("cannot publish " + path);
    }
}

bool read_uid(const std::string &path, time_t not_before, unsigned char id[128])
{
    const int fd = open(path.c_str(), O_RDONLY | O_NOFOLLOW | O_CLOEXEC);
    if (fd < 0) return false;
    struct stat st;
    char magic[8];
    const bool ok = fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_uid == getuid() && st.st_mtime >= not_before &&
                    read(fd, magic, 8) == 8 && std::memcmp(magic, kUidMagic, 8) == 0 && read(fd, id, 128) == 128;
    (void)close(fd);
    return ok;
}

} // namespace

ShellSystem::ShellSystem(const Parameters &p, const Launch &launch, unsigned flags)
    : ShellSystem(p, launch.device, launch.rank, launch.world_size, flags)
{
    if (launch.world_size > 1) {
        unsigned char id[128];
        const time_t started = time(nullptr);
        if (launch.rank == 0) {
            check(femshell_comm_unique_id(id), "femshell_comm_unique_id");
            publish_uid(launch.uid_file, id);
        } else {
            const auto t0 = std::chrono::steady_clock::now();
            while (!read_uid(launch.uid_file, started - 60, id)) {
                if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(120))
                    throw std::runtime_error("rank " + std::to_string(launch.rank) + ": no fresh RCCL id in " + launch.uid_file + " after 120 s");
                std::this_thread::sleep_for(std::chrono::milliseconds(10));
            }
        }
        comm_init(id);
        if (launch.rank == 0 && !std::getenv("FEMSHELL_KEEP_UID_FILE")) std::remove(launch.uid_file.c_str()); // every rank has joined
    }
    choose_preconditioner(p);
}

void ShellSystem::choose_preconditioner(const Parameters &p)
{
    const bool amg = p.pc_type == "gamg" || p.pc_type == "amg" || p.pc_type == "ml" || p.pc_type == "hypre" || p.pc_type == "mg";
    femshell_pc_options o;
    check(femshell_pc_defaults(amg ? FEMSHELL_PC_AMG : FEMSHELL_PC_BLOCK_JACOBI, &o), "femshell_pc_defaults");
    check(femshell_set_preconditioner(ctx_, &o), "femshell_set_preconditioner");
}

ShellSystem::~ShellSystem() { femshell_destroy(ctx_); }

void ShellSystem::comm_init(const unsigned char id[128]) { check(femshell_comm_init(ctx_, id), "femshell_comm_init"); }

void ShellSystem::set_mesh(const ShellMesh &m)
{
    n_nodes_ = m.n_nodes();
    n_elems_ = m.n_tri() + m.n_quad();
    solved_once_ = false;
    check(femshell_set_mesh(ctx_, m.n_nodes(), m.xyz.data(), m.n_tri(), m.tri.data(), m.n_quad(), m.quad.data()),
          "femshell_set_mesh");
    const std::vector<uint8_t> mask = m.dirichlet_mask();
    check(femshell_set_dirichlet(ctx_, m.n_nodes(), nullptr, mask.data()), "femshell_set_dirichlet");
    mask_ = mask;
    if (!m.loads.empty()) set_forces(m.loads);
}

void ShellSystem::set_sections(const SectionTable &t)
{
    check(femshell_set_sections(ctx_, (int32_t)t.sections.size(), t.sections.data(), t.tri_section.empty() ? nullptr : t.tri_section.data(),
                                t.quad_section.empty() ? nullptr : t.quad_section.data()),
          "femshell_set_sections");
}

void ShellSystem::set_prescribed(const Parameters &p)
{
    check_prescribed_nodes(p, n_nodes_);
    check(femshell_set_prescribed(ctx_, (int32_t)p.prescribed_nodes.size(), p.prescribed_nodes.data(), p.prescribed_values.data()),
          "femshell_set_prescribed");
}

void ShellSystem::set_element_loads(const ElementLoads &l)
{
    check(femshell_set_element_loads(ctx_, l.tri_load.empty() ? nullptr : l.tri_load.data(), l.quad_load.empty() ? nullptr : l.quad_load.data()),
          "femshell_set_element_loads");
}

void ShellSystem::set_thermal(const Parameters &p, const ThermalLoads &l)
{
    check(femshell_set_expansion(ctx_, p.alpha, (int32_t)l.section_alpha.size(), l.section_alpha.empty() ? nullptr : l.section_alpha.data()),
          "femshell_set_expansion");
    check(femshell_set_thermal(ctx_, l.tri_temp.empty() ? nullptr : l.tri_temp.data(), l.quad_temp.empty() ? nullptr : l.quad_temp.data()),
          "femshell_set_thermal");
}

void ShellSystem::set_supports(const ElasticSupports &s)
{
    if (!s.tri_k.empty() || !s.quad_k.empty())
        check(femshell_set_foundation(ctx_, s.tri_k.empty() ? nullptr : s.tri_k.data(), s.quad_k.empty() ? nullptr : s.quad_k.data()),
              "femshell_set_foundation");
    if (!s.spring_nodes.empty())
        check(femshell_set_springs(ctx_, (int32_t)s.spring_nodes.size(), s.spring_nodes.data(), s.spring_values.data()), "femshell_set_springs");
}

std::vector<double> ShellSystem::support_forces()
{
    std::vector<double> f((size_t)n_nodes_ * 6, 0.0);
    check(femshell_support_forces(ctx_, nullptr, f.data()), "femshell_support_forces");
    return f;
}

std::vector<double> ShellSystem::reactions()
{
    std::vector<double> r((size_t)n_nodes_ * 6, 0.0);
    check(femshell_reactions(ctx_, nullptr, r.data()), "femshell_reactions");
    return r;
}

void ShellSystem::nodal_resultants(std::vector<double> &nodes, std::vector<double> &elems)
{
    nodes.assign((size_t)n_nodes_ * 14, 0.0);
    elems.assign((size_t)n_elems_ * 2, 0.0);
    check(femshell_nodal_resultants(ctx_, nullptr, nodes.data(), elems.data()), "femshell_nodal_resultants");
}

std::vector<double> ShellSystem::element_resultants()
{
    std::vector<double> s((size_t)n_elems_ * 14, 0.0);
    check(femshell_element_resultants(ctx_, nullptr, s.data()), "femshell_element_resultants");
    return s;
}

SectionTable read_sections(const Parameters &p, ShellMesh &mesh)
{
    SectionTable t;
    t.sections.push_back({p.nu, p.em, p.thickness}); // section 0: every element whose tag is not listed
    std::vector<int32_t> listed; // tag of section 1 + i
    auto strip = [](std::string line) {
        const size_t h = line.find('#');
        if (h != std::string::npos) line.erase(h);
        return line;
    };
    if (!p.sections_file.empty()) {
        std::ifstream in(p.sections_file);
        if (!in) throw std::runtime_error("cannot open " + p.sections_file);
        std::string line;
        for (int no = 1; std::getline(in, line); no++) {
            std::istringstream is(strip(line));
            std::string first;
            if (!(is >> first)) continue; // blank or comment
            char *end = nullptr;
            const long tag = std::strtol(first.c_str(), &end, 10);
            femshell_section s{};
            std::string rest;
            if (*end != '\0' || !(is >> s.nu >> s.E >> s.thickness) || (is >> rest))
                throw std::runtime_error(p.sections_file + ": line " + std::to_string(no) + ": expected 'tag nu E t'");
            if (std::find(listed.begin(), listed.end(), (int32_t)tag) != listed.end())
                throw std::runtime_error(p.sections_file + ": line " + std::to_string(no) + ": tag " + std::to_string(tag) + " is listed twice");
            listed.push_back((int32_t)tag);
            t.sections.push_back(s);
            t.tags.push_back((int32_t)tag);
        }
    }
    const size_t ne = mesh.order.size();
    if (!p.section_ids_file.empty()) {
        std::ifstream in(p.section_ids_file);
        if (!in) throw std::runtime_error("cannot open " + p.section_ids_file);
        std::vector<int32_t> ids;
        std::string line;
        for (int no = 1; std::getline(in, line); no++) {
            std::istringstream is(strip(line));
            std::string tok;
            while (is >> tok) {
                char *end = nullptr;
                const long v = std::strtol(tok.c_str(), &end, 10);
                if (*end != '\0') throw std::runtime_error(p.section_ids_file + ": line " + std::to_string(no) + ": '" + tok + "' is not an integer");
                ids.push_back((int32_t)v);
            }
        }
        if (ids.size() != ne)
            throw std::runtime_error(p.section_ids_file + ": " + std::to_string(ids.size()) + " ids for " + std::to_string(ne) + " elements");
        mesh.elem_tag.swap(ids);
    }
    mesh.elem_tag.resize(ne, 0);
    mesh.sections_in_use = true;
    t.tri_section.assign((size_t)mesh.n_tri(), 0);
    t.quad_section.assign((size_t)mesh.n_quad(), 0);
    for (size_t e = 0; e < ne; e++) {
        const auto it = std::find(listed.begin(), listed.end(), mesh.elem_tag[e]);
        const int32_t s = it == listed.end() ? 0 : (int32_t)(it - listed.begin()) + 1;
        (mesh.order[e].first == 't' ? t.tri_section : t.quad_section)[(size_t)mesh.order[e].second] = s;
    }
    return t;
}

void ShellSystem::set_forces(const std::vector<double> &f6)
{
    if ((int)(f6.size() / 6) != n_nodes_) throw std::runtime_error("set_forces: need one row of 6 per mesh node");
    check(femshell_set_loads(ctx_, n_nodes_, nullptr, f6.data()), "femshell_set_loads");
}

void ShellSystem::assemble_elasticity(const std::string &system_name)
{
    // libmesh_assert_equal_to (system_name, "Elasticity"), SA:1163
    if (system_name != "Elasticity") throw std::runtime_error("assemble_elasticity: system_name must be \"Elasticity\"");
    check(femshell_assemble(ctx_), "femshell_assemble");
}

femshell_cases_info ShellSystem::solve_cases(const std::vector<double> &loads, int n_cases, double tol, int max_it, std::vector<double> &u,
                                             std::vector<femshell_case_info> &cases)
{
    if (n_cases < 1 || loads.size() != (size_t)n_cases * (size_t)n_nodes_ * 6)
        throw std::runtime_error("solve_cases: need one row of 6 per mesh node and case");
    u.assign(loads.size(), 0.0);
    cases.assign((size_t)n_cases, femshell_case_info{});
    femshell_cases_info info{};
    check(femshell_solve_cases(ctx_, n_cases, loads.data(), tol, max_it, u.data(), cases.data(), &info), "femshell_solve_cases");
    return info;
}

femshell_envelope_info ShellSystem::combination_envelope(const std::vector<double> &u, int n_cases, const std::vector<double> &factors,
                                                         std::vector<double> &env, std::vector<int32_t> &gov)
{
    if (n_cases < 1 || u.size() != (size_t)n_cases * (size_t)n_nodes_ * 6 || factors.empty() || factors.size() % (size_t)n_cases != 0)
        throw std::runtime_error("combination_envelope: need one row of 6 per mesh node and case, and one factor per case and combination");
    env.assign((size_t)n_elems_ * 6, 0.0);
    gov.assign((size_t)n_elems_ * 6, 0);
    femshell_envelope_info info{};
    check(femshell_combination_envelope(ctx_, n_cases, u.data(), nullptr, (int32_t)(factors.size() / (size_t)n_cases), factors.data(), env.data(),
                                        gov.data(), &info),
          "femshell_combination_envelope");
    return info;
}

SolveResult ShellSystem::solve(double tol, int max_it)
{
    SolveResult r;
    sols_.assign((size_t)n_nodes_ * 6, 0.0);
    // libMesh hands system.solution to KSPSolve as the initial guess (PetscLinearSolver: KSPSetInitialGuessNonzero): the first
    // solve of a system starts from zero, every later one -- the coupling iterations of fem-shell_precice.cpp:271 -- from the
    // displacements of the solve before.  FEMSHELL_WARM_START=0: every solve from zero (A/B runs)
    static const bool warm = !(std::getenv("FEMSHELL_WARM_START") && std::atoi(std::getenv("FEMSHELL_WARM_START")) == 0);
    if (warm && solved_once_) check(femshell_set_initial_guess(ctx_, nullptr), "femshell_set_initial_guess");
    check(femshell_solve(ctx_, tol, max_it, sols_.data(), &r.info), "femshell_solve");
    solved_once_ = true;
    r.iterations = (unsigned)r.info.iterations;
    r.final_residual = r.info.rel_residual;
    r.converged = r.info.converged == 1;
    return r;
}

const std::vector<double> &ShellSystem::build_solution_vector() { return sols_; }

void ShellSystem::dynamics_begin(const Parameters &p, double dt)
{
    check(femshell_set_density(ctx_, p.rho, 0, nullptr), "femshell_set_density");
    femshell_dynamics_options o;
    check(femshell_dynamics_defaults(&o), "femshell_dynamics_defaults");
    o.dt = dt;
    o.beta = p.newmark_beta;
    o.gamma = p.newmark_gamma;
    o.alpha = p.damping;
    check(femshell_dynamics_begin(ctx_, &o, nullptr, nullptr), "femshell_dynamics_begin");
    sols_.assign((size_t)n_nodes_ * 6, 0.0);
}

SolveResult ShellSystem::dynamics_step(double tol, int max_it)
{
    SolveResult r;
    check(femshell_dynamics_step(ctx_, tol, max_it, &r.info), "femshell_dynamics_step");
    sols_.assign((size_t)n_nodes_ * 6, 0.0);
    check(femshell_dynamics_state(ctx_, 1, sols_.data(), nullptr, nullptr), "femshell_dynamics_state");
    r.iterations = (unsigned)r.info.iterations;
    r.final_residual = r.info.rel_residual;
    r.converged = r.info.converged == 1;
    return r;
}

void ShellSystem::dynamics_accept() { check(femshell_dynamics_accept(ctx_), "femshell_dynamics_accept"); }

femshell_modal_info ShellSystem::modes(const Parameters &p, std::vector<double> &lambda, std::vector<double> &modes, std::vector<double> &residual)
{
    check(femshell_set_density(ctx_, p.rho, 0, nullptr), "femshell_set_density");
    femshell_modal_options o;
    check(femshell_modal_defaults(&o), "femshell_modal_defaults");
    o.n_modes = p.modes;
    o.tol = p.modes_tol;
    o.shift = p.modes_shift;
    lambda.assign((size_t)p.modes, 0.0);
    residual.assign((size_t)p.modes, 0.0);
    modes.assign((size_t)p.modes * (size_t)n_nodes_ * 6, 0.0);
    femshell_modal_info info{};
    check(femshell_modes(ctx_, &o, lambda.data(), modes.data(), residual.data(), &info), "femshell_modes");
    return info;
}

femshell_buckling_info ShellSystem::buckling(const Parameters &p, std::vector<double> &lambda, std::vector<double> &shapes, std::vector<double> &rho)
{
    femshell_buckling_options o;
    check(femshell_buckling_defaults(&o), "femshell_buckling_defaults");
    o.n_modes = p.buckling;
    o.tol = p.buckling_tol;
    lambda.assign((size_t)p.buckling, 0.0);
    rho.assign((size_t)p.buckling, 0.0);
    shapes.assign((size_t)p.buckling * (size_t)n_nodes_ * 6, 0.0);
    femshell_buckling_info info{};
    check(femshell_buckling(ctx_, &o, nullptr, lambda.data(), shapes.data(), rho.data(), &info), "femshell_buckling");
    return info;
}

namespace {
double wall_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
} // namespace

PhaseClock::PhaseClock()
{
    const char *e = std::getenv("FEMSHELL_TIMING");
    enabled_ = e && std::atoi(e) != 0;
    start_ = last_ = wall_now();
}

void PhaseClock::done(const std::string &phase)
{
    const double t = wall_now();
    phases_.emplace_back(phase, t - last_);
    last_ = t;
}

void PhaseClock::report(std::ostream &err) const
{
    if (!enabled_) return;
    char buf[64];
    err << "Times [s]:";
    for (const auto &p : phases_) {
        snprintf(buf, sizeof buf, " %.3f", p.second);
        err << " " << p.first << buf << " |";
    }
    snprintf(buf, sizeof buf, " %.3f", last_ - start_);
    err << " total" << buf;
    for (const std::string &n : notes_) err << " | " << n;
    err << std::endl;
}

int fem_shell_main(int argc, char **argv, std::ostream &out, std::ostream &err)
{
    PhaseClock clock;
    Parameters p;
    if (read_parameters(argc, argv, p, out, err)) {
        out << "Read command-line arguments.......OK" << std::endl;
    } else {
        out << "Read command-line arguments.......FAILED" << std::endl;
        return -1;
    }
    // the stand-alone program's dynamics needs all three of -rho -dt -steps (still before any device is touched)
    if (p.dynamics_requested() && (p.dt <= 0.0 || p.steps <= 0)) {
        err << "ERROR: -rho needs -dt and -steps (a number of time steps > 0)!\n";
        out << "Read command-line arguments.......FAILED" << std::endl;
        return -1;
    }
    if (!p.dynamics_requested() && (has_flag(argc, argv, "-dt") || has_flag(argc, argv, "-steps"))) {
        err << "ERROR: -dt / -steps need a density, -rho!\n";
        out << "Read command-line arguments.......FAILED" << std::endl;
        return -1;
    }
    try {
        ShellMesh mesh = read_mesh(p.in_filename);
        out << " Mesh Information:\n  n_nodes()=" << mesh.n_nodes() << "\n  n_elem()=" << mesh.n_tri() + mesh.n_quad()
            << "\n";
        // CONVENTION: force file = mesh file name without extension + "_f" (SA:42-50); a missing
        // file means no loads, as in the reference (SA:52)
        try {
            mesh.loads = read_forces(force_file_name(p.in_filename), mesh.n_nodes());
        } catch (const std::exception &) {
            mesh.loads.assign((size_t)mesh.n_nodes() * 6, 0.0);
        }
        // -load_cases: every listed file is the whole load of its case (read before any device is touched)
        std::vector<double> case_loads;
        if (p.load_cases_requested()) {
            const size_t n6 = (size_t)mesh.n_nodes() * 6;
            for (const std::string &file : p.load_case_files) {
                const std::vector<double> f = read_forces(file, mesh.n_nodes());
                if (f.size() != n6) throw std::runtime_error(file + ": expected " + std::to_string(mesh.n_nodes()) + " rows of 6");
                case_loads.insert(case_loads.end(), f.begin(), f.end());
            }
            mesh.loads.assign(n6, 0.0); // (the context's own loads play no part)
        }
        SectionTable section_table;
        if (p.sections_requested()) section_table = read_sections(p, mesh);
        if (p.prescribed_requested()) check_prescribed_nodes(p, mesh.n_nodes()); // (before any device is touched)
        ElementLoads element_loads;
        if (p.element_loads_requested()) element_loads = build_element_loads(p, mesh, p.sections_requested() ? &section_table : nullptr); // (likewise)
        ThermalLoads thermal_loads;
        if (p.thermal_requested()) thermal_loads = build_thermal_loads(p, mesh, p.sections_requested() ? &section_table : nullptr); // (likewise)
        ElasticSupports supports;
        if (p.supports_requested()) supports = build_elastic_supports(p, mesh); // (likewise)
        clock.done("read mesh and loads");
        const Launch launch = Launch::from_environment();
        ShellSystem system(p, launch);
        clock.done("context (device, ranks)");
        system.set_mesh(mesh);
        if (p.sections_requested()) system.set_sections(section_table);
        if (p.prescribed_requested()) {
            if (launch.world_size != 1) throw std::runtime_error("-prescribed runs on one rank");
            system.set_prescribed(p);
        }
        if (p.element_loads_requested()) system.set_element_loads(element_loads); // (on top of the force file's nodal loads)
        if (p.thermal_requested()) system.set_thermal(p, thermal_loads); // (on top of all other loads; after the sections: alpha belongs to them)
        if (p.supports_requested()) system.set_supports(supports); // (K + mask(K_sup) from the first assembly on: solve, time stepping, modes, buckling)
        if (p.support_forces && launch.world_size != 1) throw std::runtime_error("-support_forces runs on one rank");
        if (p.reactions && launch.world_size != 1) throw std::runtime_error("-reactions runs on one rank");
        if (p.stress && launch.world_size != 1) throw std::runtime_error("-stress runs on one rank");
        if (p.stress_nodes && launch.world_size != 1) throw std::runtime_error("-stress_nodes runs on one rank");
        if (p.buckling_requested() && launch.world_size != 1) throw std::runtime_error("-buckling runs on one rank");
        clock.done("symbolic phase, boundary conditions, loads");
        if (p.load_cases_requested()) {
            // the listed load cases in one call instead of the single solve
            if (launch.world_size != 1) throw std::runtime_error("-load_cases runs on one rank");
            const int n_cases = (int)p.load_case_files.size();
            std::vector<double> u;
            std::vector<femshell_case_info> cases;
            const femshell_cases_info ci = system.solve_cases(case_loads, n_cases, p.tol, p.max_it, u, cases);
            clock.done("assembly, preconditioner setup, load cases");
            const std::string stem = p.isOutfileSet ? p.out_filename : std::string("out");
            std::ofstream cf(stem + "_cases.txt");
            if (!cf) throw std::runtime_error("cannot write " + stem + "_cases.txt");
            const size_t n6 = (size_t)mesh.n_nodes() * 6;
            bool all_converged = true;
            for (int k = 0; k < n_cases; k++) {
                const femshell_case_info &c = cases[(size_t)k];
                char tail[96];
                snprintf(tail, sizeof tail, " %d %d %.15e\n", c.iterations, c.converged, c.rel_residual);
                cf << k + 1 << " " << p.load_case_names[(size_t)k] << tail;
                all_converged = all_converged && c.converged == 1;
                const std::vector<double> uk(u.begin() + (std::ptrdiff_t)((size_t)k * n6), u.begin() + (std::ptrdiff_t)((size_t)(k + 1) * n6));
                std::vector<PointVectors> arrays(2);
                for (int part = 0; part < 2; part++) {
                    arrays[(size_t)part].name = part == 0 ? "displacement" : "rotation";
                    arrays[(size_t)part].xyz.resize((size_t)mesh.n_nodes() * 3);
                    for (int32_t n = 0; n < mesh.n_nodes(); n++)
                        for (int d = 0; d < 3; d++) arrays[(size_t)part].xyz[3 * (size_t)n + d] = uk[6 * (size_t)n + 3 * part + d];
                }
                write_vtk(mesh, uk, stem + "_case" + std::to_string(k + 1) + ".vtk", &arrays);
                out << " case " << k + 1 << " (" << p.load_case_names[(size_t)k] << "): " << c.iterations << " iterations, ||r||/||b|| = " << c.rel_residual
                    << (c.converged == 1 ? "" : " (NOT converged)") << std::endl;
            }
            out << "Load cases: " << n_cases << " cases in " << ci.passes << (ci.passes == 1 ? " pass" : " passes") << " ("
                << (ci.pc_type == FEMSHELL_PC_AMG ? "multigrid-preconditioned CG, one case after another"
                                                  : (ci.fused_product ? "6x6 block-Jacobi CG in lockstep, one pass over K for the cases of a pass"
                                                                      : "6x6 block-Jacobi CG in lockstep"))
                << "), " << ci.solve_seconds << " s; " << stem << "_cases.txt, " << stem << "_case<k>.vtk" << std::endl;
            if (p.combinations_requested()) {
                // the envelope of the listed combinations: a line per element in the order of the mesh file (the cells of the VTK
                // file); the library's rows are the triangles, then the quadrilaterals
                std::vector<double> env;
                std::vector<int32_t> gov;
                const femshell_envelope_info ei = system.combination_envelope(u, n_cases, p.combination_factors, env, gov);
                const size_t n_combos = p.combination_factors.size() / (size_t)n_cases;
                std::ofstream ef(stem + "_envelope.txt");
                if (!ef) throw std::runtime_error("cannot write " + stem + "_envelope.txt");
                static const char *names[6] = {"von_mises_top_max", "von_mises_bottom_max", "N1_max", "N2_min", "M1_max", "M2_min"};
                ef << "# element";
                for (int k = 0; k < 6; k++) ef << " " << names[k];
                for (int k = 0; k < 6; k++) ef << " governs_" << names[k];
                ef << "\n";
                const size_t ne = mesh.order.size();
                std::vector<CellArray> arrays(12);
                for (int k = 0; k < 6; k++) {
                    arrays[(size_t)k].name = names[k];
                    arrays[(size_t)k].values.resize(ne);
                    arrays[6 + (size_t)k].name = std::string("governs_") + names[k];
                    arrays[6 + (size_t)k].values.resize(ne);
                    arrays[6 + (size_t)k].integer = true;
                }
                double worst = 0.0;
                int worst_combo = 1;
                char word[40];
                for (size_t e = 0; e < ne; e++) {
                    const size_t row = mesh.order[e].first == 't' ? (size_t)mesh.order[e].second : (size_t)mesh.n_tri() + (size_t)mesh.order[e].second;
                    ef << e;
                    for (int k = 0; k < 6; k++) {
                        snprintf(word, sizeof word, " %.15e", env[6 * row + (size_t)k]);
                        ef << word;
                        arrays[(size_t)k].values[e] = env[6 * row + (size_t)k];
                    }
                    for (int k = 0; k < 6; k++) {
                        ef << " " << gov[6 * row + (size_t)k] + 1;
                        arrays[6 + (size_t)k].values[e] = (double)(gov[6 * row + (size_t)k] + 1);
                    }
                    ef << "\n";
                    for (int k = 0; k < 2; k++)
                        if (env[6 * row + (size_t)k] > worst) {
                            worst = env[6 * row + (size_t)k];
                            worst_combo = gov[6 * row + (size_t)k] + 1;
                        }
                }
                write_vtk(mesh, std::vector<double>(n6, 0.0), stem + "_envelope.vtk", nullptr, &arrays);
                out << "Load combinations: " << n_combos << " combinations of " << n_cases << " cases, largest surface von Mises stress = " << worst
                    << " (combination " << worst_combo << "), " << ei.seconds_cases + ei.seconds_envelope << " s on the device; " << stem
                    << "_envelope.txt, " << stem << "_envelope.vtk" << std::endl;
            }
            clock.done("output files");
            out << "All done :)\n";
            clock.report(err);
            return all_converged ? 0 : 2;
        }
        if (p.modes_requested()) {
            // natural frequencies and mode shapes instead of a solve
            if (launch.world_size != 1) throw std::runtime_error("-modes runs on one rank");
            std::vector<double> lambda, shapes, residual;
            const femshell_modal_info mi = system.modes(p, lambda, shapes, residual);
            clock.done("assembly, preconditioner setup, modal analysis");
            const std::string stem = p.isOutfileSet ? p.out_filename : std::string("out");
            std::ofstream mf(stem + "_modes.txt");
            if (!mf) throw std::runtime_error("cannot write " + stem + "_modes.txt");
            const double two_pi = 6.283185307179586476925286766559;
            for (int k = 0; k < p.modes; k++) {
                char line[200];
                snprintf(line, sizeof line, "%d %.15e %.15e %.15e\n", k + 1, lambda[(size_t)k], std::sqrt(std::max(lambda[(size_t)k], 0.0)) / two_pi,
                         residual[(size_t)k]);
                mf << line;
            }
            out << "Modal analysis: " << mi.converged << " of " << p.modes << " pairs converged in " << mi.iterations << " iterations of a block of "
                << mi.block << " (" << (mi.pc_type == FEMSHELL_PC_AMG ? "multigrid" : "6x6 block-Jacobi") << " preconditioner, tolerance "
                << p.modes_tol << ", shift " << p.modes_shift << "), worst residual " << mi.residual_max << "; frequencies in " << stem
                << "_modes.txt" << std::endl;
            for (int k = 0; k < p.modes; k++)
                out << " mode " << k + 1 << ": lambda = " << lambda[(size_t)k] << ", f = " << std::sqrt(std::max(lambda[(size_t)k], 0.0)) / two_pi << std::endl;
            if (p.isOutfileSet) {
                const size_t n6 = (size_t)mesh.n_nodes() * 6;
                std::vector<PointVectors> arrays;
                for (int k = 0; k < p.modes; k++)
                    for (int part = 0; part < 2; part++) {
                        PointVectors a;
                        a.name = "mode_" + std::to_string(k + 1) + (part == 0 ? "_u" : "_r");
                        a.xyz.resize((size_t)mesh.n_nodes() * 3);
                        for (int32_t n = 0; n < mesh.n_nodes(); n++)
                            for (int d = 0; d < 3; d++) a.xyz[3 * (size_t)n + d] = shapes[(size_t)k * n6 + 6 * (size_t)n + 3 * part + d];
                        arrays.push_back(std::move(a));
                    }
                write_vtk(mesh, std::vector<double>(n6, 0.0), p.out_filename + ".vtk", &arrays);
                clock.done("output files");
            }
            out << "All done :)\n";
            clock.report(err);
            return mi.converged == p.modes ? 0 : 2;
        }
        SolveResult res;
        if (p.dynamics_requested()) {
            // the force file's loads as a step load at t = 0, from rest: p.steps Newmark steps, the probe node's history
            int32_t probe = p.probe;
            if (probe < 0) { // the node of largest load (the force's norm; the first of equals)
                probe = 0;
                double best = -1.0;
                for (int32_t n = 0; n < mesh.n_nodes(); n++) {
                    const double *f = &mesh.loads[6 * (size_t)n];
                    const double norm = std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
                    if (norm > best) {
                        best = norm;
                        probe = n;
                    }
                }
            }
            if (probe >= mesh.n_nodes()) throw std::runtime_error("-probe: the mesh has no node " + std::to_string(probe));
            system.dynamics_begin(p, p.dt);
            std::ofstream hist;
            if (launch.rank == 0) {
                hist.open((p.isOutfileSet ? p.out_filename : std::string("out")) + "_history.txt");
                if (!hist) throw std::runtime_error("cannot write the history file");
            }
            long cg_iterations = 0;
            bool all_converged = true;
            for (int n = 1; n <= p.steps; n++) {
                const SolveResult step = system.dynamics_step(p.tol, p.max_it);
                system.dynamics_accept();
                cg_iterations += step.iterations;
                all_converged = all_converged && step.converged;
                if (n == 1) res = step; // (assembly and preconditioner setup happen in the first step)
                else res.info.solve_seconds += step.info.solve_seconds;
                res.iterations = step.iterations;
                res.final_residual = step.final_residual;
                if (launch.rank == 0) {
                    const double *s = &system.build_solution_vector()[6 * (size_t)probe];
                    char line[160];
                    snprintf(line, sizeof line, "%.17g %.17g %.17g %.17g\n", n * p.dt, s[0], s[1], s[2]);
                    hist << line;
                }
            }
            res.converged = all_converged;
            if (launch.rank == 0)
                out << "Structural dynamics: " << p.steps << " Newmark steps of dt = " << p.dt << " (beta = " << p.newmark_beta << ", gamma = "
                    << p.newmark_gamma << ", damping = " << p.damping << ", rho = " << p.rho << "), " << cg_iterations
                    << " CG iterations, history of node " << probe << " in " << (p.isOutfileSet ? p.out_filename : std::string("out"))
                    << "_history.txt" << std::endl;
        } else {
            res = system.solve(p.tol, p.max_it);
        }
        clock.done("assembly, preconditioner setup, solve");
        {
            char note[160];
            snprintf(note, sizeof note, "of which assembly %.4f, preconditioner setup %.3f, iterations %.3f", res.info.assemble_seconds,
                     res.info.pc_setup_seconds, res.info.solve_seconds);
            clock.note(note);
        }
        const std::vector<double> &sols = system.build_solution_vector();
        if (launch.rank != 0) return res.converged ? 0 : 2; // every rank holds the solution (SA:141); rank 0 reports it
        out << "Linear solver: " << (res.info.pc_type == FEMSHELL_PC_AMG ? "multigrid-preconditioned" : "6x6 block-Jacobi")
            << " CG on MI355X";
        if (launch.world_size > 1) out << " (" << launch.world_size << " ranks)";
        out << ", " << res.iterations << " iterations, ||r||/||b|| = "
            << res.final_residual << (res.converged ? "" : " (NOT converged)") << std::endl;
        out << "Solution: u_vec = [";
        for (int32_t id = 0; id < mesh.n_nodes(); id++) {
            const double *s = &sols[6 * (size_t)id];
            out << "u= " << s[0] << ", v= " << s[1] << ", w= " << s[2];
            out << ", tx= " << s[3] << ", ty= " << s[4] << ", tz= " << s[5] << "]" << std::endl;
        }
        out << "]" << std::endl << std::endl;
        clock.done("print the solution");
        std::vector<PointVectors> reaction_arrays;
        if (p.reactions) {
            // what the supports carry: a line per node with a fixed dof, then the column sums over all nodes (at free dofs r is
            // the negative residual of the solve: the force columns of the sum balance the loads)
            const std::vector<double> r = system.reactions();
            const std::vector<uint8_t> &mask = system.dirichlet_mask();
            const std::string stem = p.isOutfileSet ? p.out_filename : std::string("out");
            std::ofstream rf(stem + "_reactions.txt");
            if (!rf) throw std::runtime_error("cannot write " + stem + "_reactions.txt");
            double sum[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            char line[240];
            for (int32_t n = 0; n < mesh.n_nodes(); n++) {
                const double *q = &r[6 * (size_t)n];
                for (int v = 0; v < 6; v++) sum[v] += q[v];
                if (!mask[(size_t)n]) continue;
                snprintf(line, sizeof line, "%d %.15e %.15e %.15e %.15e %.15e %.15e\n", n, q[0], q[1], q[2], q[3], q[4], q[5]);
                rf << line;
            }
            snprintf(line, sizeof line, "sum %.15e %.15e %.15e %.15e %.15e %.15e\n", sum[0], sum[1], sum[2], sum[3], sum[4], sum[5]);
            rf << line;
            out << "Support reactions: sum of the forces = (" << sum[0] << ", " << sum[1] << ", " << sum[2] << "), in " << stem << "_reactions.txt"
                << std::endl;
            for (int part = 0; part < 2; part++) {
                PointVectors a;
                a.name = part == 0 ? "reaction_f" : "reaction_m";
                a.xyz.resize((size_t)mesh.n_nodes() * 3);
                for (int32_t n = 0; n < mesh.n_nodes(); n++)
                    for (int d = 0; d < 3; d++) a.xyz[3 * (size_t)n + d] = r[6 * (size_t)n + 3 * part + d];
                reaction_arrays.push_back(std::move(a));
            }
        }
        if (p.support_forces) {
            // what the elastic supports exert on the shell, -K_sup u: a line per node, then the column sums
            const std::vector<double> f = system.support_forces();
            const std::string stem = p.isOutfileSet ? p.out_filename : std::string("out");
            std::ofstream sf(stem + "_support.txt");
            if (!sf) throw std::runtime_error("cannot write " + stem + "_support.txt");
            double sum[3] = {0.0, 0.0, 0.0};
            char line[240];
            for (int32_t n = 0; n < mesh.n_nodes(); n++) {
                const double *q = &f[6 * (size_t)n];
                for (int v = 0; v < 3; v++) sum[v] += q[v];
                snprintf(line, sizeof line, "%d %.15e %.15e %.15e %.15e %.15e %.15e\n", n, q[0], q[1], q[2], q[3], q[4], q[5]);
                sf << line;
            }
            out << "Elastic supports: sum of the forces on the shell = (" << sum[0] << ", " << sum[1] << ", " << sum[2] << "), in " << stem
                << "_support.txt" << std::endl;
            for (int part = 0; part < 2; part++) {
                PointVectors a;
                a.name = part == 0 ? "support_f" : "support_m";
                a.xyz.resize((size_t)mesh.n_nodes() * 3);
                for (int32_t n = 0; n < mesh.n_nodes(); n++)
                    for (int d = 0; d < 3; d++) a.xyz[3 * (size_t)n + d] = f[6 * (size_t)n + 3 * part + d];
                reaction_arrays.push_back(std::move(a));
            }
        }
        std::vector<CellArray> stress_arrays;
        if (p.stress) {
            // what the shell carries: a line per element in the order of the mesh file (the cells of <out>.vtk); the library's rows
            // are the triangles, then the quadrilaterals
            const std::vector<double> s = system.element_resultants();
            const std::string stem = p.isOutfileSet ? p.out_filename : std::string("out");
            std::ofstream sf(stem + "_stress.txt");
            if (!sf) throw std::runtime_error("cannot write " + stem + "_stress.txt");
            sf << "# element Nxx Nyy Nzz Nxy Nyz Nzx Mxx Myy Mzz Mxy Myz Mzx von_mises_top von_mises_bottom\n"
               << "# N: membrane force per length, M: moment per length (M = integral of sigma z dz), global axes; element means\n";
            static const char *names[4] = {"membrane_force", "moment", "von_mises_top", "von_mises_bottom"};
            static const int first[4] = {0, 6, 12, 13}, comps[4] = {6, 6, 1, 1};
            const size_t ne = mesh.order.size();
            for (int a = 0; a < 4; a++) {
                CellArray c;
                c.name = names[a];
                c.components = comps[a];
                c.values.resize(ne * (size_t)comps[a]);
                stress_arrays.push_back(std::move(c));
            }
            double worst = 0.0;
            char word[40];
            for (size_t e = 0; e < ne; e++) {
                const size_t row = mesh.order[e].first == 't' ? (size_t)mesh.order[e].second : (size_t)mesh.n_tri() + (size_t)mesh.order[e].second;
                const double *q = &s[14 * row];
                sf << e;
                for (int v = 0; v < 14; v++) {
                    snprintf(word, sizeof word, " %.15e", q[v]);
                    sf << word;
                }
                sf << "\n";
                for (int a = 0; a < 4; a++)
                    for (int v = 0; v < comps[a]; v++) stress_arrays[(size_t)a].values[e * (size_t)comps[a] + v] = q[first[a] + v];
                worst = std::max(worst, std::max(q[12], q[13]));
            }
            out << "Element resultants: largest surface von Mises stress = " << worst << ", in " << stem << "_stress.txt" << std::endl;
        }
        std::vector<CellArray> node_arrays;
        if (p.stress_nodes) {
            // the element tensors averaged to the nodes, and how far every element lies from the average: node lines in the mesh's
            // numbering, element lines in the order of the mesh file
            std::vector<double> nodes, elems;
            system.nodal_resultants(nodes, elems);
            const std::string stem = p.isOutfileSet ? p.out_filename : std::string("out");
            std::ofstream nf(stem + "_stress_nodes.txt");
            if (!nf) throw std::runtime_error("cannot write " + stem + "_stress_nodes.txt");
            nf << "# node Nxx Nyy Nzz Nxy Nyz Nzx Mxx Myy Mzz Mxy Myz Mzx W fold\n"
               << "# N, M: the element means averaged over the elements at the node with their areas, global axes; W: the sum of those areas;\n"
               << "# fold: 1 - |sum of the vector areas| / W (0: flat and consistently oriented; elsewhere the average means little)\n";
            static const char *nnames[3] = {"membrane_force_nodes", "moment_nodes", "fold"};
            static const int nfirst[3] = {0, 6, 13}, ncomps[3] = {6, 6, 1};
            const size_t nn = (size_t)mesh.n_nodes();
            for (int a = 0; a < 3; a++) {
                CellArray c;
                c.name = nnames[a];
                c.components = ncomps[a];
                c.values.resize(nn * (size_t)ncomps[a]);
                node_arrays.push_back(std::move(c));
            }
            char word[40];
            for (size_t n = 0; n < nn; n++) {
                const double *q = &nodes[14 * n];
                nf << n;
                for (int v = 0; v < 14; v++) {
                    snprintf(word, sizeof word, " %.15e", q[v]);
                    nf << word;
                }
                nf << "\n";
                for (int a = 0; a < 3; a++)
                    for (int v = 0; v < ncomps[a]; v++) node_arrays[(size_t)a].values[n * (size_t)ncomps[a] + v] = q[nfirst[a] + v];
            }
            const size_t ne = mesh.order.size();
            CellArray eta;
            eta.name = "error_indicator";
            eta.components = 1;
            eta.values.resize(ne);
            double se2 = 0.0, seta2 = 0.0; // summed in the order of the library's rows: triangles, then quadrilaterals
            for (size_t r = 0; r < ne; r++) {
                se2 += elems[2 * r];
                seta2 += elems[2 * r + 1];
            }
            const double rel = se2 + seta2 > 0.0 ? std::sqrt(seta2 / (se2 + seta2)) : 0.0;
            std::ofstream ef(stem + "_error.txt");
            if (!ef) throw std::runtime_error("cannot write " + stem + "_error.txt");
            char line[200];
            snprintf(line, sizeof line, "# sum_e2 %.15e sum_eta2 %.15e relative_error %.15e\n", se2, seta2, rel);
            ef << "# element e2 eta2\n"
               << "# e2: twice the complementary energy of the element means; eta2: the energy of the recovered field minus the element's value\n"
               << line;
            for (size_t e = 0; e < ne; e++) {
                const size_t row = mesh.order[e].first == 't' ? (size_t)mesh.order[e].second : (size_t)mesh.n_tri() + (size_t)mesh.order[e].second;
                snprintf(line, sizeof line, "%zu %.15e %.15e\n", e, elems[2 * row], elems[2 * row + 1]);
                ef << line;
                eta.values[e] = std::sqrt(elems[2 * row + 1]);
            }
            stress_arrays.push_back(std::move(eta));
            snprintf(line, sizeof line, "%.6e", rel);
            out << "Nodal resultants: relative error of the mesh = " << line << ", in " << stem << "_stress_nodes.txt and " << stem << "_error.txt"
                << std::endl;
        }
        bool buckling_converged = true;
        if (p.buckling_requested()) {
            // at what multiple of the solved load case the shell buckles, and in which shapes: the prestress is the solution's
            std::vector<double> lambda, shapes, rho;
            const femshell_buckling_info bi = system.buckling(p, lambda, shapes, rho);
            clock.done("buckling analysis");
            buckling_converged = bi.converged == p.buckling;
            const std::string stem = p.isOutfileSet ? p.out_filename : std::string("out");
            std::ofstream bf(stem + "_buckling.txt");
            if (!bf) throw std::runtime_error("cannot write " + stem + "_buckling.txt");
            bf << "# mode lambda rho\n"
               << "# lambda: load factor of (K + lambda K_G) x = 0, signed, by magnitude; rho: ||A x - mu K x||_{K^-1} / (|mu| ||x||_K), mu = 1 / lambda\n";
            for (int k = 0; k < p.buckling; k++) {
                char line[120];
                snprintf(line, sizeof line, "%d %.15e %.15e\n", k + 1, lambda[(size_t)k], rho[(size_t)k]);
                bf << line;
            }
            out << "Linear buckling: " << bi.converged << " of " << p.buckling << " pairs converged in " << bi.iterations << " iterations of a block of "
                << bi.block << " (" << bi.inner_iterations << " CG iterations of the "
                << (bi.pc_type == FEMSHELL_PC_AMG ? "multigrid-preconditioned" : "6x6 block-Jacobi") << " inner solves, tolerance " << p.buckling_tol
                << "), worst rho " << bi.rho_max << "; load factors in " << stem << "_buckling.txt" << std::endl;
            for (int k = 0; k < p.buckling; k++) out << " buckling mode " << k + 1 << ": lambda = " << lambda[(size_t)k] << std::endl;
            const size_t n6 = (size_t)mesh.n_nodes() * 6;
            for (int k = 0; k < p.buckling; k++)
                for (int part = 0; part < 2; part++) {
                    PointVectors a;
                    a.name = "buckling_" + std::to_string(k + 1) + (part == 0 ? "_u" : "_r");
                    a.xyz.resize((size_t)mesh.n_nodes() * 3);
                    for (int32_t n = 0; n < mesh.n_nodes(); n++)
                        for (int d = 0; d < 3; d++) a.xyz[3 * (size_t)n + d] = shapes[(size_t)k * n6 + 6 * (size_t)n + 3 * part + d];
                    reaction_arrays.push_back(std::move(a)); // (the point arrays of <out>.vtk: reactions, then buckling shapes)
                }
        }
        if (p.isOutfileSet) {
            write_exodus(mesh, sols, p.out_filename + ".e"); // the reference's file (fem-shell.cpp:1249)
            write_vtk(mesh, sols, p.out_filename + ".vtk", reaction_arrays.empty() ? nullptr : &reaction_arrays, stress_arrays.empty() ? nullptr : &stress_arrays,
                      node_arrays.empty() ? nullptr : &node_arrays);
            clock.done("output files");
        }
        out << "All done :)\n";
        clock.report(err);
        return res.converged && buckling_converged ? 0 : 2;
    } catch (const std::exception &e) {
        err << "ERROR: " << e.what() << std::endl;
        return 1;
    }
}

} // namespace femshell_host
