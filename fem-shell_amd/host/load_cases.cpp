// load_cases.cpp -- see load_cases.hpp
#include "load_cases.hpp"

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
