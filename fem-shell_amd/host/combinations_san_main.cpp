// combinations_san_main.cpp -- the reader of FEM-shell -combinations FILE2 under AddressSanitizer and UBSan (`make san`): exactly
// read_combinations of load_cases.cpp, with no library and no GPU behind it.
//     combinations_san FILE2 N_CASES
// prints "<n_combos> combinations of <n_cases> cases", then one line of factors (%.17g) per combination; a refused file: the
// message on stderr and exit status 1.  The sanitizers end the program themselves on a finding.
#include "load_cases.hpp"

#include <cstdio>
#include <cstdlib>
#include <exception>
#include <iostream>

int main(int argc, char **argv)
{
    const int n_cases = argc == 3 ? std::atoi(argv[2]) : 0;
    if (n_cases < 1 || n_cases > femshell_host::kMaxLoadCases) {
        std::cerr << "usage: combinations_san FILE2 N_CASES (1 .. " << femshell_host::kMaxLoadCases << ")\n";
        return 2;
    }
    try {
        const std::vector<double> f = femshell_host::read_combinations(argv[1], n_cases);
        const size_t n_combos = f.size() / (size_t)n_cases;
        std::cout << n_combos << " combinations of " << n_cases << " cases\n";
        for (size_t c = 0; c < n_combos; c++) {
            for (int j = 0; j < n_cases; j++) std::printf("%s%.17g", j ? " " : "", f[c * (size_t)n_cases + (size_t)j]);
            std::printf("\n");
        }
    } catch (const std::exception &e) {
        std::cerr << "ERROR: " << e.what() << "\n";
        return 1;
    }
    return 0;
}
