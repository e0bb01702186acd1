// load_cases_san_main.cpp -- the host-only parts of FEM-shell -load_cases under AddressSanitizer and UBSan (`make san`): the list
// reader and the option check of load_cases.cpp, with no library and no GPU behind them.
//     load_cases_san LIST [further command-line words ...]
// prints the files of the list, one per line as "<name> -> <path>", then "conflicts: <flags>"; a refused list: the message on
// stderr and exit status 1.  The sanitizers end the program themselves on a finding.
#include "load_cases.hpp"

#include <exception>
#include <iostream>

int main(int argc, char **argv)
{
    if (argc < 2) {
        std::cerr << "usage: load_cases_san LIST [further command-line words ...]\n";
        return 2;
    }
    try {
        std::vector<std::string> names;
        const std::vector<std::string> files = femshell_host::read_load_cases_list(argv[1], &names);
        for (size_t i = 0; i < files.size(); i++) std::cout << names[i] << " -> " << files[i] << "\n";
    } catch (const std::exception &e) {
        std::cerr << "ERROR: " << e.what() << "\n";
        return 1;
    }
    std::cout << "conflicts: " << femshell_host::load_cases_conflicts(argc - 1, argv + 1) << "\n";
    return 0;
}
