// dev_pool.hpp -- the device memory of the library's buffers: DevPool (arenas, kept blocks, deferred frees) and DevBuf<T> on top
// of it.  Nothing here dereferences device memory: pointer arithmetic and seven HIP calls (hipMalloc, hipFree,
// hipDeviceSynchronize, hipGetDevice, hipSetDevice, hipGetLastError, hipMemset), so tests/helpers/pool_main.cpp drives it on a CPU
// against a driver of its own, and tests/helpers/pool_model.py judges the trace (the rules: DESIGN.md, "The device pool").
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <map>
#include <mutex>
#include <unordered_map>
#include <utility>
#include <vector>

#include "knobs.hpp"

namespace femshell {

// FEMSHELL_POOL_VERBOSE=1: every hipMalloc of the pool below goes to stderr with its size and time (read per call)
inline bool pool_verbose() { return knob_flag("FEMSHELL_POOL_VERBOSE", false); }

// Device memory of the library's buffers.
// (1) ARENAS (round 6).  A multigrid setup at 4M triangles makes about 150 allocations, and hipMalloc costs 0.5 - 2.5 ms a call on
//     the boxes of this pool whatever the size: 60 to 370 ms of a 0.18 - 0.5 s setup were the driver's allocator
//     (FEMSHELL_AMG_VERBOSE=1 prints the count).  Requests below kArenaMax are therefore carved out of arenas of kArenaBytes (one
//     hipMalloc each, bump pointer, 256-byte granules); larger ones -- K's values, the big operators -- go to the driver as before.
// (2) REUSE.  Blocks a buffer gives back are kept (per device) and handed to the next request of about their size: a setup
//     allocates and frees about 10 GB of transient operators (P, A P, R, A_c, Q), every setup after the first of a process -- a
//     changed K in a coupled run, the next context of a test process -- finds them here.  Directly allocated blocks of 1 MiB and
//     more are kept up to FEMSHELL_POOL_GB gigabytes (default 24; 0 = no pool and no arenas), pieces of arenas always (they cannot go
//     back to the driver one by one).  A block is reused only after the device IT BELONGS TO has gone idle once since it came back
//     (hipFree synchronises too); everything goes back to the driver when the last context of the process is destroyed, and
//     nothing is kept while no context is open.
// What holds FEMSHELL_POOL_GB: the kept blocks (cached_bytes()) and the kept blocks that were carved ((3) below) count against it
// whenever no Defer object is alive.  A carved block nothing of which is in use is a kept block again -- it can serve a request
// of its whole size, and it can go back to the driver.  Only the arenas the pool asked the driver for as arenas stay outside the
// limit, until an out-of-memory answer or the last context takes them.
// What a small buffer can pin: a request below kArenaMax is never placed in a block of the driver's that is larger than one
// arena -- neither as the first piece of a carved block nor in the room a large request left in one -- so a 256-byte buffer
// holds at most FEMSHELL_POOL_ARENA_MB, not the 3 to 26 GB of a returned A P.
class DevPool {
  public:
    static constexpr size_t kMinBytes = 1u << 20;
    static constexpr size_t kGranule = 256;
    static constexpr size_t kArenaMax = 96u << 20; // requests below this come out of an arena

    static DevPool &get()
    {
        static DevPool pool;
        return pool;
    }
    // FEMSHELL_POOL_POISON=1 (tests, debugging): every block is filled with 0xFF bytes -- NaNs as doubles and floats, -1 as
    // integers -- before it is handed out.  Fresh memory from the driver is zero and recycled memory is not: whoever relies on
    // zeros it never wrote works until the pool hands it a used block (found that way: round 6, the carved blocks).
    hipError_t alloc(void **out, size_t bytes)
    {
        const hipError_t e = alloc_raw(out, bytes);
        if (e == hipSuccess && poison_ && *out != nullptr && bytes > 0) {
            (void)hipMemset(*out, 0xFF, bytes);
            (void)hipDeviceSynchronize();
        }
        return e;
    }
    // (a request of no bytes gets no block: nullptr and hipSuccess, no call of the driver)
    hipError_t alloc_raw(void **out, size_t bytes)
    {
        *out = nullptr;
        if (bytes == 0) return hipSuccess;
        int dev = 0;
        if (limit_ > 0) (void)hipGetDevice(&dev);
        const bool small = limit_ > 0 && arena_bytes_ > 0 && bytes < kArenaMax;
        const size_t need = small ? (bytes + kGranule - 1) / kGranule * kGranule : bytes;
        if (limit_ > 0 && (small || bytes >= kMinBytes)) {
            std::lock_guard<std::mutex> lock(m_);
            // best fit: the smallest kept block of this device that holds the request without wasting more than a quarter
            // (for a small request: not a piece of a carved block larger than one arena, see "what a small buffer can pin")
            const size_t most = need + need / 4 + (small ? kGranule : 0);
            for (auto it = free_.lower_bound(Key{dev, need}); it != free_.end() && it->first.dev == dev && it->first.bytes <= most; ++it) {
                Arena *in = arena_of(it->second);
                if (small && in != nullptr && in->bytes > arena_bytes_) continue;
                *out = it->second;
                live_[*out] = Block{it->first.bytes, dev, true};
                live_bytes_ += it->first.bytes;
                if (in == nullptr) cached_ -= it->first.bytes;
                else in->live++;
                free_.erase(it);
                return hipSuccess;
            }
            if (small) {
                Arena *a = nullptr;
                for (auto &kv : arenas_) {
                    Arena &ar = kv.second;
                    if (ar.dev == dev && ar.bytes <= arena_bytes_ && ar.used + need <= ar.bytes) {
                        a = &ar;
                        break;
                    }
                }
                if (a == nullptr && carve_) // (a kept block of the driver's of at most one arena that holds the request becomes the next arena)
                    for (auto jt = free_.lower_bound(Key{dev, need}); jt != free_.end() && jt->first.dev == dev && jt->first.bytes <= arena_bytes_; ++jt) {
                        if (in_arena(jt->second)) continue;
                        a = carve(jt);
                        break;
                    }
                if (a == nullptr) {
                    void *base = nullptr;
                    const size_t ab = arena_bytes_;
                    const auto t0 = std::chrono::steady_clock::now();
                    const hipError_t e = hipMalloc(&base, ab);
                    stat_malloc_ns_ += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
                    stat_mallocs_++;
                    if (pool_verbose()) fprintf(stderr, "[femshell pool] hipMalloc of an arena, %zu MB (for a request of %zu bytes)\n", ab >> 20, bytes);
                    if (e == hipSuccess) {
                        outstanding_ += ab;
                        a = new_arena(dev, static_cast<char *>(base), ab, false);
                    } else {
                        (void)hipGetLastError(); // (no room for another arena: the request goes to the driver on its own, below)
                    }
                }
                if (a != nullptr) {
                    *out = bump(a, need, dev);
                    return hipSuccess;
                }
            } else if (arena_bytes_ > 0 && carve_) {
                // (3) CARVING (round 6).  A large request that no kept block fits within a quarter: (a) room in a block that was
                // carved before, else (b) the smallest kept block that holds it at all becomes an arena and the request its first
                // piece; the rest serves the LARGE requests that follow.  A multigrid setup ends with the single-precision copies --
                // 1.1, 0.8, 0.7 GB at 4M triangles -- right after A P (3.1 GB) has come back: five hipMalloc calls and 2.6 GB of fresh
                // memory less, which is 35-50 ms on a box whose allocator is in its slow state (profiles/r06_hipmalloc_probe.txt).
                // When its last piece comes back the block is a kept block again (keep_block).
                const size_t need_g = (bytes + kGranule - 1) / kGranule * kGranule;
                Arena *a = nullptr;
                for (auto &kv : arenas_) {
                    Arena &ar = kv.second;
                    if (ar.carved && ar.dev == dev && ar.used + need_g <= ar.bytes) {
                        a = &ar;
                        break;
                    }
                }
                if (a == nullptr)
                    for (auto jt = free_.lower_bound(Key{dev, need_g}); jt != free_.end() && jt->first.dev == dev; ++jt) {
                        if (in_arena(jt->second)) continue;
                        a = carve(jt);
                        break;
                    }
                if (a != nullptr) {
                    *out = bump(a, need_g, dev);
                    return hipSuccess;
                }
            }
        }
        const auto t0 = std::chrono::steady_clock::now();
        hipError_t e = hipMalloc(out, bytes);
        stat_malloc_ns_ += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
        stat_mallocs_++;
        if (pool_verbose())
            fprintf(stderr, "[femshell pool] hipMalloc %.1f MB: %.2f ms\n", (double)bytes / 1048576.0,
                    1e-6 * (double)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count());
        if (e != hipSuccess) { // out of memory: whatever nothing lives in (kept, waiting for the end of a setup, idle arenas) goes back, one more try
            (void)hipGetLastError();
            const bool waited = flush_pending(), kept = trim();
            if (waited || kept) {
                e = hipMalloc(out, bytes);
                if (e != hipSuccess) (void)hipGetLastError();
            }
        }
        if (e == hipSuccess) {
            std::lock_guard<std::mutex> lock(m_);
            live_[*out] = Block{bytes, dev, bytes >= kMinBytes && limit_ > 0};
            live_bytes_ += bytes;
            outstanding_ += bytes;
        } else {
            *out = nullptr;
        }
        return e;
    }
    void free(void *p)
    {
        if (p == nullptr) return;
        const auto t0 = std::chrono::steady_clock::now();
        Block b{0, 0, false};
        bool arena = false, known = false;
        int dev = 0;
        {
            std::lock_guard<std::mutex> lock(m_);
            auto it = live_.find(p);
            if (it != live_.end()) {
                known = true;
                b = it->second;
                live_.erase(it);
                live_bytes_ -= b.bytes;
                const Arena *a = arena_of(p);
                arena = a != nullptr;
                dev = arena ? a->dev : b.dev; // (the device the block belongs to, whichever is current now)
                // (a block too large to keep, released inside a multigrid setup -- A P of a 32M-triangle mesh, 26 GB -- waits with the
                //  others: freed at once, the setup's NEXT requests -- the single-precision copies -- waited for the driver to wipe it,
                //  0.65 s of hipMalloc in a 1.05 s setup; kept until the setup is over it is what those requests are carved from)
                // (decided and queued under the one lock: the Defer that ends meanwhile finds the block in its flush, or this sees no Defer)
                if ((arena || b.kept) && defer_depth_.load() > 0) { // (a multigrid setup in progress: see Defer below)
                    pending_.push_back(Pending{p, b.bytes, arena, dev});
                    return;
                }
                if (!arena && (!b.kept || b.bytes > limit_)) outstanding_ -= b.bytes; // (back to the driver, below)
            }
        }
        if (!known || (!arena && (!b.kept || b.bytes > limit_))) {
            (void)hipFree(p);
            stat_free_ns_ += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
            stat_frees_++;
            return;
        }
        sync_device(dev); // (what hipFree does: nothing in flight reads or writes the block any more)
        stat_sync_ns_ += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
        stat_syncs_++;
        std::lock_guard<std::mutex> lock(m_);
        keep_block(p, b.bytes, arena, dev);
        if (contexts_.load() == 0) (void)trim_locked();
    }
    // While a Defer object lives, blocks that come back to the pool wait in a list instead of synchronising the device one by one
    // (the power iteration of a multigrid setup runs on the second stream from the setup's first moment; a temporary buffer of the
    // search for clusters, released 1 ms in, used to wait 22 ms for it).  They are not handed out again before the last Defer object
    // is gone: one synchronisation per device then, and they join the kept blocks.
    struct Defer {
        Defer() { DevPool::get().defer_depth_.fetch_add(1); }
        ~Defer()
        {
            if (DevPool::get().defer_depth_.fetch_sub(1) == 1) {
                (void)DevPool::get().flush_pending();
                DevPool::get().enforce_limit();
            }
        }
        Defer(const Defer &) = delete;
        Defer &operator=(const Defer &) = delete;
    };
    // (when the last Defer object is gone: kept blocks beyond the pool's limit go back to the driver, largest first; all of them
    //  when the last context was closed meanwhile)
    void enforce_limit()
    {
        std::lock_guard<std::mutex> lock(m_);
        trim_to_limit();
        if (contexts_.load() == 0) (void)trim_locked();
    }
    bool flush_pending()
    {
        std::vector<Pending> list;
        {
            std::lock_guard<std::mutex> lock(m_);
            list.swap(pending_);
        }
        if (list.empty()) return false;
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<int> devs; // (every device a block of the list belongs to goes idle once; the caller's device is current again after)
        for (const Pending &b : list)
            if (std::find(devs.begin(), devs.end(), b.dev) == devs.end()) devs.push_back(b.dev);
        for (int d : devs) sync_device(d);
        stat_sync_ns_ += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
        stat_syncs_ += list.size();
        std::lock_guard<std::mutex> lock(m_);
        for (const Pending &b : list) keep_block(b.p, b.bytes, b.arena, b.dev);
        return true;
    }

  private:
    struct Pending {
        void *p;
        size_t bytes;
        bool arena;
        int dev;
    };
    static void sync_device(int dev)
    {
        int cur = dev;
        (void)hipGetDevice(&cur);
        if (cur != dev) (void)hipSetDevice(dev);
        (void)hipDeviceSynchronize();
        if (cur != dev) (void)hipSetDevice(cur);
    }
    // (callers hold m_; the block's device has been idle since the block came back)
    void keep_block(void *p, size_t bytes, bool arena, int dev)
    {
        if (arena) {
            Arena *a = arena_of(p);
            a->live--;
            if (a->live == 0) { // nothing of it in use: its kept pieces leave the free list, and ...
                for (auto it = free_.begin(); it != free_.end();)
                    if (a->holds(it->second)) it = free_.erase(it);
                    else ++it;
                if (!a->carved) { // ... an arena starts over,
                    a->used = 0;
                    return;
                }
                // ... a carved block is a kept block of the driver's again: counted, reusable as a whole, returnable
                const Key whole{a->dev, a->bytes};
                char *base = a->base;
                arena_total_ -= whole.bytes;
                carved_bytes_ -= whole.bytes;
                arenas_.erase(base);
                free_.emplace(whole, base);
                cached_ += whole.bytes;
                if (defer_depth_.load() == 0) trim_to_limit();
                return;
            }
            free_.emplace(Key{a->dev, bytes}, p);
            return;
        }
        free_.emplace(Key{dev, bytes}, p);
        cached_ += bytes;
        if (defer_depth_.load() > 0) return; // (inside a setup the kept blocks may exceed the limit: enforce_limit() when it is over)
        trim_to_limit();
    }
    void trim_to_limit()
    {
        while (cached_ + carved_bytes_ > limit_) { // over the limit: the largest kept block that is the driver's goes back to it
            auto big = free_.end();
            for (auto it = free_.end(); it != free_.begin();) {
                --it;
                if (!in_arena(it->second)) {
                    big = it;
                    break;
                }
            }
            if (big == free_.end()) break;
            cached_ -= big->first.bytes;
            outstanding_ -= big->first.bytes;
            (void)hipFree(big->second);
            free_.erase(big);
        }
    }
    bool trim_locked()
    {
        bool any = false;
        for (auto it = free_.begin(); it != free_.end();) {
            if (in_arena(it->second)) {
                ++it;
                continue;
            }
            outstanding_ -= it->first.bytes;
            (void)hipFree(it->second);
            it = free_.erase(it);
            any = true;
        }
        cached_ = 0;
        for (auto ar = arenas_.begin(); ar != arenas_.end();) {
            const Arena &a = ar->second;
            if (a.live != 0) {
                ++ar;
                continue;
            }
            for (auto it = free_.begin(); it != free_.end();)
                if (a.holds(it->second)) it = free_.erase(it);
                else ++it;
            outstanding_ -= a.bytes;
            arena_total_ -= a.bytes;
            if (a.carved) carved_bytes_ -= a.bytes;
            (void)hipFree(a.base);
            ar = arenas_.erase(ar);
            any = true;
        }
        return any;
    }

  public:
    // every kept block back to the driver, and every arena nothing of which is in use; true when there was one
    bool trim()
    {
        std::lock_guard<std::mutex> lock(m_);
        return trim_locked();
    }
    void context_opened() { contexts_.fetch_add(1); }
    void context_closed()
    {
        if (contexts_.fetch_sub(1) == 1) { // (blocks a setup left waiting on a path that did not flush them go back as well)
            (void)flush_pending();
            (void)trim();
        }
    }
    // (FEMSHELL_AMG_VERBOSE: what the driver's allocator cost since the last call -- hipMalloc, hipFree, the synchronisations of
    //  blocks that went back to the pool)
    void stats(double out[6])
    {
        out[0] = (double)stat_mallocs_.exchange(0);
        out[1] = 1e-6 * (double)stat_malloc_ns_.exchange(0);
        out[2] = (double)stat_frees_.exchange(0);
        out[3] = 1e-6 * (double)stat_free_ns_.exchange(0);
        out[4] = (double)stat_syncs_.exchange(0);
        out[5] = 1e-6 * (double)stat_sync_ns_.exchange(0);
    }
    size_t cached_bytes()
    {
        std::lock_guard<std::mutex> lock(m_);
        return cached_;
    }
    // (femshell_pool_stats: bytes the driver has handed to the pool and not got back, bytes in use, cached_bytes(), number of
    //  arenas -- carved blocks among them -- and their bytes, blocks waiting for the end of a setup)
    void counters(double out[6])
    {
        std::lock_guard<std::mutex> lock(m_);
        out[0] = (double)outstanding_;
        out[1] = (double)live_bytes_;
        out[2] = (double)cached_;
        out[3] = (double)arenas_.size();
        out[4] = (double)arena_total_;
        out[5] = (double)pending_.size();
    }
    size_t limit_bytes() const { return limit_; }
    size_t arena_bytes() const { return arena_bytes_; }

  private:
    struct Key {
        int dev;
        size_t bytes;
        bool operator<(const Key &o) const { return dev != o.dev ? dev < o.dev : bytes < o.bytes; }
    };
    struct Block { // a block in use
        size_t bytes;
        int dev;
        bool kept; // comes back to the pool (false: below kMinBytes from the driver directly, or no pool: straight to hipFree)
    };
    struct Arena {
        int dev;
        char *base;
        size_t bytes, used;
        int64_t live; // pieces in use
        bool carved = false; // a kept block turned into an arena (alloc (3)); large requests are served from these only
        bool holds(const void *p) const { return static_cast<const char *>(p) >= base && static_cast<const char *>(p) < base + bytes; }
    };
    DevPool()
    {
        const double gb = knob_double("FEMSHELL_POOL_GB", 24.0);
        limit_ = gb > 0.0 ? (size_t)(gb * 1073741824.0) : 0;
        poison_ = knob_flag("FEMSHELL_POOL_POISON", false);
        carve_ = knob_flag("FEMSHELL_POOL_CARVE", true); // (0: no carving of kept blocks, A/B runs)
        const double mb = knob_double("FEMSHELL_POOL_ARENA_MB", 512.0); // 0: no arenas (every request to the driver, as in round 5)
        arena_bytes_ = mb > 0.0 ? std::max((size_t)(mb * 1048576.0), 2 * kArenaMax) : 0;
    }
    // (callers hold m_)
    Arena *arena_of(const void *p)
    {
        auto it = arenas_.upper_bound(static_cast<char *>(const_cast<void *>(p)));
        if (it == arenas_.begin()) return nullptr;
        --it;
        return it->second.holds(p) ? &it->second : nullptr;
    }
    bool in_arena(const void *p) { return arena_of(p) != nullptr; }
    Arena *new_arena(int dev, char *base, size_t bytes, bool carved)
    {
        arena_total_ += bytes;
        if (carved) carved_bytes_ += bytes;
        return &arenas_.emplace(base, Arena{dev, base, bytes, 0, 0, carved}).first->second;
    }
    // the kept block at `jt` becomes an arena
    Arena *carve(std::multimap<Key, void *>::iterator jt)
    {
        Arena *a = new_arena(jt->first.dev, static_cast<char *>(jt->second), jt->first.bytes, true);
        cached_ -= jt->first.bytes;
        free_.erase(jt);
        return a;
    }
    void *bump(Arena *a, size_t need, int dev)
    {
        void *p = a->base + a->used;
        a->used += need;
        a->live++;
        live_[p] = Block{need, dev, true};
        live_bytes_ += need;
        return p;
    }
    std::mutex m_;
    std::multimap<Key, void *> free_;
    std::unordered_map<void *, Block> live_;
    std::map<char *, Arena> arenas_; // by base address (a map: the pointers into it stay valid)
    size_t cached_ = 0, limit_ = 0, arena_bytes_ = 0;
    size_t outstanding_ = 0, live_bytes_ = 0, arena_total_ = 0, carved_bytes_ = 0;
    bool poison_ = false, carve_ = true;
    std::atomic<int> contexts_{0}, defer_depth_{0};
    std::vector<Pending> pending_;
    std::atomic<uint64_t> stat_mallocs_{0}, stat_malloc_ns_{0}, stat_frees_{0}, stat_free_ns_{0}, stat_syncs_{0}, stat_sync_ns_{0};
};

template <class T> struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    ~DevBuf() { release(); }
    // owns its block: moves, never copies
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept { swap(o); }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) {
            release();
            swap(o);
        }
        return *this;
    }
    void swap(DevBuf &o) noexcept
    {
        std::swap(p, o.p);
        std::swap(n, o.n);
    }
    void release()
    {
        if (p) DevPool::get().free(p);
        p = nullptr;
        n = 0;
    }
    hipError_t alloc(size_t count)
    {
        if (count == n && p) return hipSuccess;
        release();
        if (count == 0) return hipSuccess;
        hipError_t e = DevPool::get().alloc(reinterpret_cast<void **>(&p), count * sizeof(T));
        if (e == hipSuccess) n = count;
        return e;
    }
    template <class Vec> hipError_t upload(const Vec &h, hipStream_t st) // any contiguous container of T
    {
        hipError_t e = alloc(h.size());
        if (e != hipSuccess || h.empty()) return e;
        return hipMemcpyAsync(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, st);
    }
    hipError_t zero(hipStream_t st) { return n ? hipMemsetAsync(p, 0, n * sizeof(T), st) : hipSuccess; }
};

} // namespace femshell
