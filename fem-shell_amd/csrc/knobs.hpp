// knobs.hpp -- how the library reads its environment switches, and the only place in csrc/ that calls
// getenv.  Host only, plain C++17: the same text compiles into the HIP objects, the -x c++ objects and the host-only build.
// One rule for all of them: unset gives the default, set text is parsed by atol / atof, so text that is no number gives 0.
// Callers keep their own clamps and range checks, and decide themselves when to read (once per process: static const).
#pragma once

#include <cstdlib>
#include <cstring>

namespace femshell {

inline const char *knob_text(const char *name) { return std::getenv(name); } // the raw text, or null

inline long knob_long(const char *name, long dflt)
{
    const char *e = knob_text(name);
    return e ? std::atol(e) : dflt;
}

inline double knob_double(const char *name, double dflt)
{
    const char *e = knob_text(name);
    return e ? std::atof(e) : dflt;
}

inline bool knob_flag(const char *name, bool dflt) // (=0 switches a default-on flag off, any other number a default-off one on)
{
    const char *e = knob_text(name);
    return e ? std::atol(e) != 0 : dflt;
}

inline bool knob_is(const char *name, const char *text) // set, and exactly that text
{
    const char *e = knob_text(name);
    return e && std::strcmp(e, text) == 0;
}

} // namespace femshell
