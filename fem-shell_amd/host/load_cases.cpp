// load_cases.cpp -- see load_cases.hpp
#include "load_cases.hpp"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>

namespace femshell_host {

std::vector<std::string> read_load_cases_list(const std::string &list_file, std::vector<std::string> *names)
{
    std::ifstream in(list_file);
    if (!in) throw std::runtime_error("cannot open " + list_file);
    const size_t slash = list_file.rfind('/');
    const std::string dir = slash == std::string::npos ? std::string() : list_file.substr(0, slash + 1);
    std::vector<std::string> files;
    if (names) names->clear();
    std::string line;
    for (int no = 1; std::getline(in, line); no++) {
        const size_t h = line.find('#');
        if (h != std::string::npos) line.erase(h);
        std::istringstream is(line);
        std::string word, rest;
        if (!(is >> word)) continue; // blank or comment
        const std::string where = list_file + ": line " + std::to_string(no) + ": ";
        if (is >> rest) throw std::runtime_error(where + "expected one force file per line");
        if ((int)files.size() == kMaxLoadCases)
            throw std::runtime_error(where + "more than " + std::to_string(kMaxLoadCases) + " load cases");
        const std::string path = word[0] == '/' ? word : dir + word;
        if (!std::ifstream(path)) throw std::runtime_error(where + "cannot open " + path);
        files.push_back(path);
        if (names) names->push_back(word);
    }
    if (files.empty()) throw std::runtime_error(list_file + ": the list names no force file");
    return files;
}

std::vector<double> read_combinations(const std::string &file, int n_cases)
{
    std::ifstream in(file);
    if (!in) throw std::runtime_error("cannot open " + file);
    std::vector<double> factors;
    int n_combos = 0;
    std::string line;
    for (int no = 1; std::getline(in, line); no++) {
        const size_t h = line.find('#');
        if (h != std::string::npos) line.erase(h);
        std::istringstream is(line);
        std::string word;
        int count = 0;
        const std::string where = file + ": line " + std::to_string(no) + ": ";
        while (is >> word) {
            char *end = nullptr;
            const double v = std::strtod(word.c_str(), &end);
            if (end == word.c_str() || *end != '\0') throw std::runtime_error(where + "'" + word + "' is not a number");
            if (!std::isfinite(v)) throw std::runtime_error(where + "'" + word + "' is not a finite number");
            if (count == 0 && n_combos == kMaxCombinations)
                throw std::runtime_error(where + "more than " + std::to_string(kMaxCombinations) + " combinations");
            factors.push_back(v);
            count++;
        }
        if (count == 0) continue; // blank or comment
        if (count != n_cases)
            throw std::runtime_error(where + "expected " + std::to_string(n_cases) + " factors, one per load case, found " + std::to_string(count));
        n_combos++;
    }
    if (n_combos == 0) throw std::runtime_error(file + ": the file holds no combination");
    return factors;
}

std::string load_cases_conflicts(int argc, char **argv)
{
    static const char *const flags[] = {"-modes", "-buckling", "-dt", "-steps", "-prescribed", "-reactions", "-stress", "-stress_nodes",
                                        "-support_forces", "-pressure", "-element_loads", "-gravity", "-alpha", "-section_alpha",
                                        "-temperature", "-temperature_gradient", "-thermal"};
    std::string found;
    for (const char *f : flags)
        for (int i = 1; i < argc; i++)
            if (std::strcmp(argv[i], f) == 0) {
                found += (found.empty() ? "" : " ") + std::string(f);
                break;
            }
    return found;
}

} // namespace femshell_host
