// load_cases.hpp -- the host side of FEM-shell -load_cases FILE that needs neither a mesh nor the library: the reader of the list
// file and the check of the options a list of load cases does not go together with.  Kept apart from shell_system.cpp so that the
// sanitizer program of `make san` (load_cases_san_main.cpp) compiles exactly what the program runs.
#pragma once

#include <string>
#include <vector>

namespace femshell_host {

constexpr int kMaxLoadCases = 32; // femshell_solve_cases takes 1 .. 32 cases

// FILE lists one force file per line, each in the format of the `_f` file (mesh_io.hpp read_forces).  The conventions of the
// -prescribed reader: '#' starts a comment, blank lines are skipped, every message names the file and the line.  A path that does
// not start with '/' is taken relative to the directory of the list file.  Throws std::runtime_error for a list that cannot be
// opened, a line with more than one word, a listed file that cannot be opened, an empty list and more than kMaxLoadCases cases.
// Returns the paths as the program opens them; names (when given): the words as the list has them, for <out>_cases.txt.
std::vector<std::string> read_load_cases_list(const std::string &list_file, std::vector<std::string> *names = nullptr);

// The options -load_cases does not go together with: another analysis or output of the single solve (-modes, -buckling, -dt,
// -steps, -prescribed, -reactions, -stress, -stress_nodes, -support_forces) and every other source of loads (-pressure,
// -element_loads, -gravity, -alpha, -section_alpha, -temperature, -temperature_gradient, -thermal): a case is its force file and
// nothing else.  Returns the offending flags, separated by blanks; empty: none.
std::string load_cases_conflicts(int argc, char **argv);

constexpr int kMaxCombinations = 256; // femshell_combination_envelope takes 1 .. 256 combinations

// -combinations FILE2: one load combination per line, exactly n_cases numbers each -- the factors of the cases in the order of
// the list of -load_cases.  The conventions of the list reader: '#' starts a comment, blank lines are skipped, every token is
// parsed whole, every message names the file and the line.  Throws std::runtime_error for a file that cannot be opened, a line
// with another count of numbers, a token that is no number or not finite, a file without a combination and more than
// kMaxCombinations lines.  Returns the factors row by row, n_combos x n_cases.
std::vector<double> read_combinations(const std::string &file, int n_cases);

} // namespace femshell_host
