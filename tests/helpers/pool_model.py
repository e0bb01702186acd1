"""The rules of the device-memory pool (csrc/dev_pool.hpp, DESIGN.md "The device pool"), checked on a trace of
tests/helpers/pool_main.cpp with interval bookkeeping only: which driver allocations are outstanding, which blocks the caller
holds, which byte ranges came back since their device last went idle.  Nothing here knows how the pool finds a block -- arenas,
free lists, best fit -- so it cannot share a mistake with it.  All rules are exact.

    1 placement   a block lies inside one outstanding driver allocation of the current device, has the requested size at least,
                  overlaps no block in use, and is non-null (a request of 0 bytes: null, and no driver call)
    2 idle        no byte of a block handed out came back since the last synchronisation of its device
    3 poison      FEMSHELL_POOL_POISON=1: memset 0xFF over the whole block, then a synchronisation, right before every hand-out
    4 no leak     no free of an address the driver does not own, none of an allocation with a block in use; nothing outstanding
                  once no context is open, no Defer alive and no block in use; nothing waiting without a Defer
    5 limit       without a Defer: the driver allocations with no block in use, other than those asked for as arenas, add up to
                  cached_bytes() and to FEMSHELL_POOL_GB at most
    6 reclaim     a refused request of n bytes: n plus the allocations with a block in use exceeds the capacity, every other
                  allocation has gone back, and hipGetLastError has been consumed
    7 pinning     a request below the arena threshold never lies in a driver allocation larger than one arena
    8 devices     rules 1 and 2 per device; the caller's current device is the same after an operation as before it
"""
import bisect


class Op:
    __slots__ = ("index", "text", "words", "events", "res", "st")

    def __init__(self, index, text):
        self.index, self.text, self.words, self.events, self.res, self.st = index, text, text.split(), [], None, {}

    def count(self, kind):
        return sum(1 for e in self.events if e[0] == kind)


def parse(text):
    """(consts, [Op]) of a trace"""
    consts, ops = {}, []
    for line in text.splitlines():
        w = line.split()
        if not w:
            continue
        if w[0] == "consts":
            consts = {k: int(v) for k, v in (x.split("=") for x in w[1:])}
        elif w[0] == "op":
            ops.append(Op(len(ops), line[3:]))
        elif w[0] == "ev":
            ops[-1].events.append((w[1],) + tuple(int(x) for x in w[2:]))
        elif w[0] == "res":
            ops[-1].res = int(w[2]) if w[1] == "ok" else (None if w[1] == "-" else "err")
        elif w[0] == "st":
            ops[-1].st = {k: int(v) for k, v in (x.split("=") for x in w[1:])}
        else:
            raise ValueError("not a line of a pool trace: " + line)
    return consts, ops


class Alloc:
    __slots__ = ("base", "bytes", "dev", "as_arena", "in_use")

    def __init__(self, base, nbytes, dev, as_arena):
        self.base, self.bytes, self.dev, self.as_arena, self.in_use = base, nbytes, dev, as_arena, 0


class Model:
    DEFAULT_CAPACITY = 64 << 30

    def __init__(self, consts, poison=False):
        self.c, self.poison = consts, poison
        self.pooled = consts["limit"] > 0
        self.arenas_on = self.pooled and consts["arena"] > 0
        self.allocs, self.bases = {}, []   # driver allocations by base, and the sorted bases
        self.live = {}                     # id -> (addr, bytes, dev, Alloc or None)
        self.spans = []                    # sorted (addr, end) of the blocks in use
        self.dirty = []                    # (dev, lo, hi) given back, device not idle since
        self.dev, self.defers, self.contexts = 0, 0, 0
        self.capacity = {}
        self.violations = []               # (rule, op index, text)
        self.kinds = {"fresh arena": 0, "arena": 0, "kept": 0, "carved": 0, "direct": 0, "refused": 0}
        self.handouts = []                 # (op index, kind)

    # ------------------------------------------------------------ helpers
    def bad(self, rule, op, text):
        self.violations.append((rule, op.index, "rule %d at operation %d (%s): %s" % (rule, op.index, op.text, text)))

    def containing(self, addr):
        i = bisect.bisect_right(self.bases, addr) - 1
        if i < 0:
            return None
        a = self.allocs[self.bases[i]]
        return a if addr < a.base + a.bytes else None

    def outstanding(self):
        return sum(a.bytes for a in self.allocs.values())

    def pinned(self, dev):
        return sum(a.bytes for a in self.allocs.values() if a.dev == dev and a.in_use > 0)

    def _event(self, op, e, request):
        if e[0] == "malloc":
            _, dev, base, nbytes = e
            if dev != self.dev:
                self.bad(8, op, "hipMalloc on device %d while %d is current" % (dev, self.dev))
            as_arena = self.arenas_on and request is not None and request < self.c["arena_max"] and nbytes == self.c["arena"]
            self.allocs[base] = Alloc(base, nbytes, dev, as_arena)
            bisect.insort(self.bases, base)
        elif e[0] == "free":
            _, dev, base, nbytes = e
            a = self.allocs.pop(base, None)
            if a is None:
                self.bad(4, op, "hipFree of %d, which the driver does not own" % base)
                return
            self.bases.remove(base)
            if a.in_use > 0:
                self.bad(4, op, "hipFree of an allocation with %d blocks in use" % a.in_use)
            self.dirty = [d for d in self.dirty if not (a.base <= d[1] < a.base + a.bytes)]  # (hipFree synchronises)
        elif e[0] == "badfree":
            self.bad(4, op, "hipFree of %d, which the driver does not own" % e[1])
        elif e[0] == "sync":
            self.dirty = [d for d in self.dirty if d[0] != e[1]]

    # ------------------------------------------------------------ one operation
    def step(self, op):
        w = op.words
        request = int(w[2]) if w[0] == "alloc" else None
        if w[0] == "free" and int(w[1]) not in self.live:  # (its request was refused, or asked for 0 bytes)
            if op.events:
                self.bad(4, op, "driver events for an id that holds no block")
        elif w[0] == "free":
            addr, nbytes, dev, a = self.live.pop(int(w[1]))
            self.spans.remove((addr, addr + nbytes))
            if a is not None:
                a.in_use -= 1
            self.dirty.append((dev, addr, addr + nbytes))
        elif w[0] == "dev":
            self.dev = int(w[1])
        elif w[0] == "cap":
            self.capacity[int(w[1])] = int(w[2])
        elif w[0] == "open":
            self.contexts += 1
        elif w[0] == "close":
            self.contexts -= 1
        elif w[0] == "defer+":
            self.defers += 1
        elif w[0] == "defer-":
            self.defers -= 1
        pinned_before = self.pinned(self.dev) if w[0] == "alloc" else 0
        for e in op.events:
            self._event(op, e, request)
        if w[0] == "alloc":
            self._handout(op, int(w[1]), request, pinned_before)
        self._after(op)

    def _handout(self, op, ident, n, pinned_before):
        cap = self.capacity.get(self.dev, self.DEFAULT_CAPACITY)
        if op.res == "err":
            self.kinds["refused"] += 1
            if n + pinned_before <= cap:
                self.bad(6, op, "refused although %d bytes + %d in allocations with blocks in use fit the capacity %d" % (n, pinned_before, cap))
            idle = [a for a in self.allocs.values() if a.in_use == 0]
            if idle:
                self.bad(6, op, "refused with %d allocations (%d bytes) in which nothing is in use still at the driver" % (len(idle), sum(a.bytes for a in idle)))
            return
        addr = op.res
        if n == 0:
            if addr != 0 or op.events:
                self.bad(1, op, "a request of 0 bytes got address %d and %d driver events" % (addr, len(op.events)))
            return
        if addr == 0:
            self.bad(1, op, "null block for %d bytes" % n)
            return
        a = self.containing(addr)
        if a is None or addr + n > a.base + a.bytes:
            self.bad(1, op, "block [%d, +%d) does not lie inside one outstanding driver allocation" % (addr, n))
            a = None
        elif a.dev != self.dev:
            self.bad(8, op, "block of device %d handed out while device %d is current" % (a.dev, self.dev))
        i = bisect.bisect_left(self.spans, (addr, 0))
        if (i < len(self.spans) and self.spans[i][0] < addr + n) or (i > 0 and self.spans[i - 1][1] > addr):
            self.bad(1, op, "block [%d, +%d) overlaps a block in use" % (addr, n))
        for d in self.dirty:
            if d[1] < addr + n and addr < d[2]:
                self.bad(2, op, "block [%d, +%d) overlaps [%d, %d), given back with no synchronisation of device %d since" % (addr, n, d[1], d[2], d[0]))
                break
        if self.poison:
            ok = len(op.events) >= 2 and op.events[-2] == ("memset", self.dev, addr, 255, n) and op.events[-1] == ("sync", self.dev)
            if not ok:
                self.bad(3, op, "no memset of 0xFF over the whole block followed by a synchronisation: %r" % (op.events[-2:],))
        elif op.count("memset"):
            self.bad(3, op, "memset without FEMSHELL_POOL_POISON")
        if a is not None:
            if self.arenas_on and n < self.c["arena_max"] and a.bytes > self.c["arena"]:
                self.bad(7, op, "%d bytes placed in a driver allocation of %d bytes, larger than an arena (%d)" % (n, a.bytes, self.c["arena"]))
            a.in_use += 1
            fresh = [e for e in op.events if e[0] == "malloc" and e[2] == a.base]
            # (for the counts only: a kept block is handed out whole when it wastes a quarter at most, + a granule below the threshold)
            small = self.arenas_on and n < self.c["arena_max"]
            need = -(-n // self.c["granule"]) * self.c["granule"] if small else n
            if fresh:
                kind = "fresh arena" if a.as_arena else "direct"
            elif a.as_arena:
                kind = "arena"
            elif addr == a.base and a.bytes <= need + need // 4 + (self.c["granule"] if small else 0):
                kind = "kept"
            else:
                kind = "carved"
            self.kinds[kind] += 1
            self.handouts.append((op.index, kind))
        self.live[ident] = (addr, n, self.dev, a)
        bisect.insort(self.spans, (addr, addr + n))

    def _after(self, op):
        st = op.st
        if st["dev"] != self.dev:
            self.bad(8, op, "the current device is %d after the operation, %d before" % (st["dev"], self.dev))
        if st["lasterr"] != 0:
            self.bad(6, op, "hipGetLastError would still answer %d" % st["lasterr"])
        if st["out"] != self.outstanding():
            self.bad(5, op, "the pool counts %d bytes at the driver, the driver %d" % (st["out"], self.outstanding()))
        if st["live"] < sum(s[1] - s[0] for s in self.spans):
            self.bad(5, op, "the pool counts %d bytes in use, the caller holds %d" % (st["live"], sum(s[1] - s[0] for s in self.spans)))
        if self.defers > 0:
            return
        if st["pending"] != 0:
            self.bad(4, op, "%d blocks waiting for the end of a setup, and no Defer alive" % st["pending"])
        idle = [a for a in self.allocs.values() if a.in_use == 0]
        outside = sum(a.bytes for a in idle if not a.as_arena)
        if outside > self.c["limit"]:
            self.bad(5, op, "%d bytes held outside arenas with nothing of them in use, the limit is %d" % (outside, self.c["limit"]))
        if st["cached"] != outside:
            self.bad(5, op, "cached_bytes() = %d, held outside arenas with nothing of them in use: %d" % (st["cached"], outside))
        if self.contexts == 0 and not self.live and self.allocs:
            self.bad(4, op, "%d bytes at the driver with no context open and nothing in use" % self.outstanding())


def replay(text, poison=False):
    """the model after the whole trace; model.violations lists what broke, model.ops the parsed operations"""
    consts, ops = parse(text)
    m = Model(consts, poison)
    m.ops = ops
    for op in ops:
        m.step(op)
    return m
