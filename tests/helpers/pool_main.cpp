// pool_main.cpp -- DevPool (csrc/dev_pool.hpp) on a CPU: the seven HIP calls the pool makes are defined here, over an address space
// that is never dereferenced, and the pool is driven either by a script on stdin (every operation answers with the driver events it
// caused, in order, its result and the pool's counters: tests/helpers/pool_model.py judges that trace) or by threads
// (`pool_main threads N SEED`, for the thread sanitizer).  Built by tests/test_pool_cpu.py, never loaded into Python.
//
// Script, one operation per line:  open | close | alloc ID BYTES | free ID | defer+ | defer- | flush | trim | dev N | cap DEV BYTES
// Answer per operation:            "op <the line>", then "ev malloc DEV ADDR BYTES" | "ev free DEV ADDR BYTES" | "ev badfree ADDR" |
//                                  "ev sync DEV" | "ev memset DEV ADDR VALUE BYTES" ..., then "res ok ADDR" | "res err" | "res -", then
//                                  "st dev=D lasterr=E out=.. live=.. cached=.. arenas=.. arena_bytes=.. pending=.."
// The first line printed is "consts granule=.. min=.. arena_max=.. arena=.. limit=..".
#include <hip/hip_runtime.h>

#include <atomic>
#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <memory>
#include <mutex>
#include <random>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "dev_pool.hpp"

namespace {

constexpr int kDevices = 4;
struct FakeDevice {
    size_t capacity = (size_t)64 << 30, used = 0;
    uintptr_t next = 0;
    std::map<uintptr_t, size_t> blocks;
};
std::mutex g_m;
FakeDevice g_dev[kDevices];
bool g_log = true;
std::vector<std::string> g_events;
thread_local int t_device = 0;
thread_local hipError_t t_last = hipSuccess;

void event(const char *fmt, ...)
{
    if (!g_log) return;
    char buf[160];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_events.push_back(buf);
}

int device_of(uintptr_t a) // (callers hold g_m) addresses of device d start at (d + 1) << 50
{
    const int d = (int)(a >> 50) - 1;
    return d >= 0 && d < kDevices ? d : -1;
}

} // namespace

extern "C" {

hipError_t hipMalloc(void **ptr, size_t size)
{
    std::lock_guard<std::mutex> lock(g_m);
    *ptr = nullptr;
    if (size == 0) return hipSuccess;
    FakeDevice &D = g_dev[t_device];
    if (size > D.capacity || D.used > D.capacity - size) return t_last = hipErrorOutOfMemory;
    if (D.next == 0) D.next = (uintptr_t)(t_device + 1) << 50;
    const uintptr_t a = D.next; // (never handed out twice: what the pool reuses, it reuses itself)
    D.next += (size + 4095) / 4096 * 4096 + 4096;
    D.blocks[a] = size;
    D.used += size;
    *ptr = reinterpret_cast<void *>(a);
    event("ev malloc %d %" PRIuPTR " %zu", t_device, a, size);
    return hipSuccess;
}

hipError_t hipFree(void *ptr)
{
    std::lock_guard<std::mutex> lock(g_m);
    if (ptr == nullptr) return hipSuccess;
    const uintptr_t a = reinterpret_cast<uintptr_t>(ptr);
    const int d = device_of(a);
    if (d < 0 || g_dev[d].blocks.count(a) == 0) {
        event("ev badfree %" PRIuPTR, a);
        if (!g_log) {
            fprintf(stderr, "hipFree of an address the driver does not own\n");
            abort();
        }
        return t_last = hipErrorInvalidValue;
    }
    const size_t size = g_dev[d].blocks[a];
    g_dev[d].blocks.erase(a);
    g_dev[d].used -= size;
    event("ev free %d %" PRIuPTR " %zu", d, a, size);
    return hipSuccess;
}

hipError_t hipDeviceSynchronize(void)
{
    std::lock_guard<std::mutex> lock(g_m);
    event("ev sync %d", t_device);
    return hipSuccess;
}

hipError_t hipGetDevice(int *device)
{
    *device = t_device;
    return hipSuccess;
}

hipError_t hipSetDevice(int device)
{
    if (device < 0 || device >= kDevices) return t_last = hipErrorInvalidDevice;
    t_device = device;
    return hipSuccess;
}

hipError_t hipGetLastError(void)
{
    const hipError_t e = t_last;
    t_last = hipSuccess;
    return e;
}

hipError_t hipMemset(void *dst, int value, size_t bytes)
{
    std::lock_guard<std::mutex> lock(g_m);
    event("ev memset %d %" PRIuPTR " %d %zu", t_device, reinterpret_cast<uintptr_t>(dst), value & 0xFF, bytes);
    return hipSuccess;
}

} // extern "C"

namespace {

using femshell::DevPool;

void print_state()
{
    double c[6];
    DevPool::get().counters(c);
    if ((size_t)c[2] != DevPool::get().cached_bytes()) {
        printf("counters() and cached_bytes() disagree\n");
        exit(3);
    }
    printf("st dev=%d lasterr=%d out=%.0f live=%.0f cached=%.0f arenas=%.0f arena_bytes=%.0f pending=%.0f\n", t_device, (int)t_last,
           c[0], c[1], c[2], c[3], c[4], c[5]);
}

int run_script()
{
    DevPool &pool = DevPool::get();
    printf("consts granule=%zu min=%zu arena_max=%zu arena=%zu limit=%zu\n", DevPool::kGranule, DevPool::kMinBytes, DevPool::kArenaMax,
           pool.arena_bytes(), pool.limit_bytes());
    std::map<long, void *> blocks;
    std::vector<std::unique_ptr<DevPool::Defer>> defers;
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream in(line);
        std::string op;
        in >> op;
        std::string res = "res -";
        g_events.clear();
        if (op == "open") pool.context_opened();
        else if (op == "close") pool.context_closed();
        else if (op == "alloc") {
            long id = 0;
            size_t bytes = 0;
            in >> id >> bytes;
            void *p = nullptr;
            const hipError_t e = pool.alloc(&p, bytes);
            if (e == hipSuccess) {
                blocks[id] = p;
                res = "res ok " + std::to_string(reinterpret_cast<uintptr_t>(p));
            } else {
                res = "res err";
            }
        } else if (op == "free") {
            long id = 0;
            in >> id;
            auto it = blocks.find(id); // (an id whose request was refused holds no block: nothing happens)
            if (it != blocks.end()) {
                pool.free(it->second);
                blocks.erase(it);
            }
        } else if (op == "defer+") defers.emplace_back(new DevPool::Defer());
        else if (op == "defer-") {
            if (defers.empty()) {
                fprintf(stderr, "script: defer- without defer+\n");
                return 2;
            }
            defers.pop_back();
        } else if (op == "flush") (void)pool.flush_pending();
        else if (op == "trim") (void)pool.trim();
        else if (op == "dev") {
            int d = 0;
            in >> d;
            if (hipSetDevice(d) != hipSuccess) return 2;
        } else if (op == "cap") {
            int d = 0;
            size_t bytes = 0;
            in >> d >> bytes;
            if (d < 0 || d >= kDevices) return 2;
            g_dev[d].capacity = bytes;
        } else {
            fprintf(stderr, "script: unknown operation '%s'\n", op.c_str());
            return 2;
        }
        printf("op %s\n", line.c_str());
        for (const std::string &e : g_events) printf("%s\n", e.c_str());
        printf("%s\n", res.c_str());
        print_state();
    }
    return 0;
}

// threads N SEED: N threads allocate and free at once, thread 0 opens and closes Defer objects meanwhile; no two blocks in use may
// overlap, nothing may be left waiting after the last Defer, and nothing at the driver after the last context
struct Overlap {
    std::mutex m;
    std::map<uintptr_t, size_t> live;
    bool add(uintptr_t a, size_t n)
    {
        std::lock_guard<std::mutex> lock(m);
        auto next = live.lower_bound(a);
        if (next != live.end() && next->first < a + n) return false;
        if (next != live.begin()) {
            auto prev = std::prev(next);
            if (prev->first + prev->second > a) return false;
        }
        live[a] = n;
        return true;
    }
    void remove(uintptr_t a)
    {
        std::lock_guard<std::mutex> lock(m);
        live.erase(a);
    }
};

int run_threads(int n_threads, unsigned seed)
{
    g_log = false;
    DevPool &pool = DevPool::get();
    pool.context_opened();
    Overlap overlap;
    std::atomic<int> failures{0};
    auto work = [&](int t) {
        std::mt19937_64 rng(seed * 1000003u + (unsigned)t);
        std::vector<std::pair<void *, size_t>> mine;
        std::unique_ptr<DevPool::Defer> defer;
        for (int step = 0; step < 4000 && failures.load() == 0; step++) {
            if (t == 0 && step % 37 == 0) {
                if (defer) defer.reset();
                else defer.reset(new DevPool::Defer());
            }
            const bool grow = mine.size() < 24 && (mine.empty() || rng() % 100 < 55);
            if (grow) {
                const unsigned k = (unsigned)(rng() % 100);
                size_t bytes = k < 40 ? 1 + rng() % 4096 : k < 80 ? 1 + rng() % (4u << 20) : k < 95 ? (1u << 20) + rng() % (95u << 20) : (96u << 20) + rng() % (160u << 20);
                void *p = nullptr;
                if (pool.alloc(&p, bytes) != hipSuccess) continue;
                if (p == nullptr || !overlap.add(reinterpret_cast<uintptr_t>(p), bytes)) {
                    fprintf(stderr, "thread %d: block %p of %zu bytes is null or overlaps a block in use\n", t, p, bytes);
                    failures++;
                    break;
                }
                mine.emplace_back(p, bytes);
            } else {
                const size_t i = rng() % mine.size();
                overlap.remove(reinterpret_cast<uintptr_t>(mine[i].first));
                pool.free(mine[i].first);
                mine[i] = mine.back();
                mine.pop_back();
            }
        }
        defer.reset();
        for (auto &b : mine) {
            overlap.remove(reinterpret_cast<uintptr_t>(b.first));
            pool.free(b.first);
        }
    };
    std::vector<std::thread> threads;
    for (int t = 0; t < n_threads; t++) threads.emplace_back(work, t);
    for (auto &th : threads) th.join();
    if (failures.load() != 0) return 1;
    double c[6];
    pool.counters(c);
    if (c[5] != 0.0 || c[1] != 0.0) {
        fprintf(stderr, "after the last Defer: %.0f blocks waiting, %.0f bytes in use\n", c[5], c[1]);
        return 1;
    }
    pool.context_closed();
    pool.counters(c);
    size_t at_driver = 0;
    for (const FakeDevice &D : g_dev) at_driver += D.used;
    if (at_driver != 0 || c[0] != 0.0 || c[2] != 0.0 || c[3] != 0.0) {
        fprintf(stderr, "after the last context: %zu bytes at the driver, counters %.0f %.0f %.0f\n", at_driver, c[0], c[2], c[3]);
        return 1;
    }
    printf("threads ok\n");
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc == 4 && strcmp(argv[1], "threads") == 0) return run_threads(atoi(argv[2]), (unsigned)atoi(argv[3]));
    if (argc != 1) {
        fprintf(stderr, "usage: pool_main < script   |   pool_main threads N SEED\n");
        return 2;
    }
    return run_script();
}
