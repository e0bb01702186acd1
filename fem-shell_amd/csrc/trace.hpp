// trace.hpp -- roctx ranges around the phases of the library (tracing): they show up as named spans in
// `rocprofv3 --marker-trace` / rocprof timelines and cost two library calls otherwise.
#pragma once

#include <chrono>
#include <roctracer/roctx.h>

namespace femshell {

// seconds on the steady clock: what the phases of the library time themselves with
inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct TraceRange {
    explicit TraceRange(const char *name) { roctxRangePushA(name); }
    ~TraceRange() { roctxRangePop(); }
    TraceRange(const TraceRange &) = delete;
    TraceRange &operator=(const TraceRange &) = delete;
};

} // namespace femshell
