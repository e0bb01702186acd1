"""The device-memory pool (csrc/dev_pool.hpp) without a GPU: a stand-alone program (tests/helpers/pool_main.cpp) drives the pool
against a driver of its own, built once with the address and undefined-behaviour sanitizers and once with the thread sanitizer,
and tests/helpers/pool_model.py judges every step of the trace by the rules of DESIGN.md ("The device pool").  All rules are
exact: there is no tolerance in this file.  The pool reads its knobs once per process, so every configuration is a process."""
import os
import random
import subprocess

import pytest

from tests.helpers import pool_model
from tests.helpers.product import ROOT

MiB, GiB, GB = 1 << 20, 1 << 30, 10 ** 9
GRANULE, MIN_BYTES, ARENA_MAX = 256, 1 << 20, 96 << 20   # (what the program reports as its constants is checked against these)


def _build(tmp, name, sanitize):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__"] + sanitize +
                          ["-I", os.path.join(ROOT, "fem-shell_amd", "csrc"), "-I", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"),
                           os.path.join(ROOT, "tests", "helpers", "pool_main.cpp"), "-o", exe, "-lpthread"])
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pool")
    return {"asan": _build(tmp, "pool_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]),
            "tsan": _build(tmp, "pool_tsan", ["-fsanitize=thread"])}


KNOBS = ("FEMSHELL_POOL_GB", "FEMSHELL_POOL_ARENA_MB", "FEMSHELL_POOL_CARVE", "FEMSHELL_POOL_POISON", "FEMSHELL_POOL_VERBOSE")


def run(programs, script, **knobs):
    """the model after the script ran in a process of its own with FEMSHELL_POOL_<KNOB> = value; sanitizer reports fail here"""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update({"FEMSHELL_POOL_" + k: str(v) for k, v in knobs.items()})
    r = subprocess.run([programs["asan"]], input="\n".join(script) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    m = pool_model.replay(r.stdout, poison=str(knobs.get("POISON", "0")) != "0")
    assert (m.c["granule"], m.c["min"], m.c["arena_max"]) == (GRANULE, MIN_BYTES, ARENA_MAX)
    assert len(m.ops) == sum(1 for line in script if line and not line.startswith("#"))
    return m


def clean(m):
    assert not m.violations, "%d violations, the first:\n%s" % (len(m.violations), "\n".join(v[2] for v in m.violations[:12]))
    return m


# ------------------------------------------------------------------ the setup-like cycle (rule 9, and 1 to 8 on the way)

TRANSIENTS = [3100 * 10 ** 6, 1400 * 10 ** 6, 900 * 10 ** 6, 300 * 10 ** 6, 120 * 10 ** 6]
COPIES = [1100 * 10 ** 6, 800 * 10 ** 6, 700 * 10 ** 6]


def cycle_script(repetitions):
    """what a multigrid setup asks of the pool, per repetition: transients and 100 small buffers inside a Defer, the transients
    back, flush_pending(), the three single-precision copies, the end of the Defer; then everything back"""
    rng = random.Random(7)
    small = [rng.choice([1, 40, 256, 4096, 70000, 300000, 3 * MiB]) for _ in range(100)]
    s, marks = ["open"], []
    for r in range(repetitions):
        first = len(s)
        s.append("defer+")
        s += ["alloc %d %d" % (i, b) for i, b in enumerate(TRANSIENTS)]
        s += ["alloc %d %d" % (100 + i, b) for i, b in enumerate(small)]
        s += ["free %d" % i for i in range(len(TRANSIENTS))]
        s.append("flush")
        copies = len(s)
        s += ["alloc %d %d" % (50 + i, b) for i, b in enumerate(COPIES)]
        s.append("defer-")
        s += ["free %d" % (50 + i) for i in range(len(COPIES))] + ["free %d" % (100 + i) for i in range(len(small))]
        marks.append((first, copies, len(s)))
    s.append("close")
    return s, marks


def test_setup_cycle_reaches_a_steady_state_without_the_driver(programs):
    """Rule 9 with a limit that holds one setup's transients (5.82 GB + one arena < 24 GB): from the second repetition on no
    hipMalloc at all and no growth at the driver; in every repetition the copies that follow flush_pending() come out of the
    blocks that just came back.  (With FEMSHELL_POOL_GB=4, below, rule 5 itself forbids keeping 5.82 GB between repetitions,
    so only the second half of rule 9 can hold there.)"""
    script, marks = cycle_script(8)
    m = clean(run(programs, script, GB=24))
    out_after = []
    for r, (first, copies, end) in enumerate(marks):
        mallocs = sum(op.count("malloc") for op in m.ops[first:end])
        assert (mallocs > 0) == (r == 0), "repetition %d: %d hipMalloc calls" % (r, mallocs)
        assert sum(op.count("malloc") for op in m.ops[copies:copies + 3]) == 0
        kinds = [k for i, k in m.handouts if copies <= i < copies + 3]
        assert "carved" in kinds and "direct" not in kinds, kinds
        out_after.append(m.ops[end - 1].st["out"])
    assert len(set(out_after)) == 1 and out_after[0] == sum(TRANSIENTS) + m.c["arena"], out_after
    assert m.ops[-1].st["out"] == 0


def test_setup_cycle_under_a_limit_smaller_than_its_transients(programs):
    """FEMSHELL_POOL_GB=4, the configuration in which 4.9 GB sat in carved blocks outside the limit and outside the count: with
    nothing in use the driver holds 4 GB + the arena at most after every repetition, and the copies still cause no hipMalloc"""
    script, marks = cycle_script(8)
    m = clean(run(programs, script, GB=4))
    for first, copies, end in marks:
        assert sum(op.count("malloc") for op in m.ops[copies:copies + 3]) == 0
        st = m.ops[end - 1].st
        assert st["out"] <= 4 * GiB + m.c["arena"] and st["cached"] == st["out"] - m.c["arena"], st
    assert m.ops[-1].st["out"] == 0


# ------------------------------------------------------------------ random scripts (rules 1 to 8, rule 10)

def random_script(seed, n_ops, limit, capacity, devices=2):
    """alloc / free / Defer / flush / trim / device switches over the size classes that take different branches of alloc_raw:
    below one granule, below kMinBytes, arena-sized, direct, and beyond the pool's limit"""
    rng = random.Random(seed)
    s = ["open"] + ["cap %d %d" % (d, capacity) for d in range(devices)]
    live, next_id, defers = [], 0, 0
    for _ in range(n_ops):
        x = rng.random()
        if x < 0.50 and len(live) < 60:
            k = rng.random()
            if k < 0.25:
                n = rng.randint(1, 255)
            elif k < 0.50:
                n = rng.randint(256, MIN_BYTES - 1)
            elif k < 0.75:
                n = rng.randint(MIN_BYTES, ARENA_MAX - 1)
            elif k < 0.95:
                n = rng.randint(ARENA_MAX, 700 * MiB)
            else:
                n = rng.randint(limit + 1, limit + 300 * MiB)
            if rng.random() < 0.3 and k >= 0.5:   # (sizes that come again: what finds a kept block)
                n = rng.choice([8 * MiB, 64 * MiB, 100 * MiB, 128 * MiB, 250 * MiB, 400 * MiB])
            s.append("alloc %d %d" % (next_id, n))
            live.append(next_id)
            next_id += 1
        elif x < 0.88 and live:
            s.append("free %d" % live.pop(rng.randrange(len(live))))
        elif x < 0.91:
            if defers and rng.random() < 0.6:
                s.append("defer-")
                defers -= 1
            elif defers < 2:
                s.append("defer+")
                defers += 1
        elif x < 0.94:
            s.append("flush")
        elif x < 0.95:
            s.append("trim")
        elif x < 0.99:
            s.append("dev %d" % rng.randrange(devices))
    s += ["defer-"] * defers + ["free %d" % i for i in live] + ["close"]
    return s


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_scripts_keep_every_rule(programs, seed):
    """two devices of 6 GB, a limit of 2 GB, arenas of 192 MiB: requests are refused, blocks are kept, carved, trimmed.  Every
    branch of alloc_raw must have been taken, or the script proves nothing about it."""
    m = clean(run(programs, random_script(seed, 3000, 2 * GiB, 6 * GiB), GB=2, ARENA_MB=192))
    print(seed, m.kinds)
    for kind, count in m.kinds.items():
        assert count > 0, "the script never reached: " + kind
    assert m.ops[-1].st["out"] == 0


def test_random_script_with_poison(programs):
    m = clean(run(programs, random_script(4, 1500, 2 * GiB, 6 * GiB), GB=2, ARENA_MB=192, POISON=1))
    assert sum(op.count("memset") for op in m.ops) == sum(m.kinds[k] for k in m.kinds if k != "refused") > 0


@pytest.mark.parametrize("knobs", [{"GB": 0}, {"GB": 2, "ARENA_MB": 0}, {"GB": 2, "ARENA_MB": 192, "CARVE": 0}],
                         ids=["no_pool", "no_arenas", "no_carving"])
def test_random_script_with_a_part_switched_off(programs, knobs):
    """rule 10: rules 1 to 6 hold with the pool, the arenas or the carving switched off; without a pool every request is one
    hipMalloc and every release one hipFree, and nothing else"""
    m = clean(run(programs, random_script(5, 2000, 2 * GiB, 6 * GiB), **knobs))
    if knobs.get("GB") == 0:
        for op in m.ops:
            want = [("malloc",)] if op.words[0] == "alloc" and op.res != "err" else [("free",)] if op.words[0] == "free" and op.events else []
            assert [e[:1] for e in op.events] == want, (op.text, op.events)
        assert sum(op.count("free") for op in m.ops) == sum(op.count("malloc") for op in m.ops) > 0
    if "CARVE" in knobs:
        assert m.kinds["carved"] == 0 and m.kinds["kept"] > 0 and m.kinds["arena"] > 0
    if knobs.get("ARENA_MB") == 0:
        assert m.kinds["carved"] == 0 and m.kinds["arena"] == 0 and m.kinds["fresh arena"] == 0 and m.kinds["kept"] > 0


# ------------------------------------------------------------------ directed scripts, one per rule

def test_sizes_around_the_granule_and_an_arena_filled_to_its_last_granule(programs):
    """rule 1 at 0, 1, 255, 256, 257 bytes, and at the end of an arena: 192 MiB = 95 + 95 + 2 MiB - 256 + 256 bytes"""
    sizes = [0, 1, 255, 256, 257]
    s = ["open"] + ["alloc %d %d" % (i, n) for i, n in enumerate(sizes)] + ["free %d" % i for i in range(len(sizes))]
    s += ["alloc 10 %d" % (95 * MiB), "alloc 11 %d" % (95 * MiB), "alloc 12 %d" % (2 * MiB - 256), "alloc 13 256", "alloc 14 1"]
    s += ["free %d" % i for i in range(10, 15)] + ["close"]
    m = clean(run(programs, s, ARENA_MB=192))
    a = [op.res for op in m.ops[1:6]]
    assert a[0] == 0 and [a[i + 1] - a[i] for i in range(1, 4)] == [256, 256, 256]   # (257 bytes take two granules: checked by the next hand-out, 10)
    arena = 192 * MiB
    assert [op.count("malloc") for op in m.ops[11:16]] == [0, 0, 0, 0, 1], "the first arena holds 10 to 13 exactly, 14 opens the next"
    assert m.ops[14].res + 256 == a[1] + arena and m.ops[11].res == a[1]   # (13 is the last granule; the arena started over for 10)
    assert m.ops[-1].st["out"] == 0


def test_arena_threshold(programs):
    """kArenaMax - 1 bytes come out of an arena, kArenaMax bytes from the driver on their own"""
    m = clean(run(programs, ["open", "alloc 0 %d" % (ARENA_MAX - 1), "alloc 1 %d" % ARENA_MAX, "free 0", "free 1", "close"]))
    assert [k for _, k in m.handouts] == ["fresh arena", "direct"]
    assert m.ops[1].events[0][3] == 512 * MiB and m.ops[2].events[0][3] == ARENA_MAX


def test_keep_threshold_without_arenas(programs):
    """kMinBytes - 1 goes back to the driver at once, kMinBytes is kept and handed out again"""
    s = ["open", "alloc 0 %d" % (MIN_BYTES - 1), "free 0", "alloc 1 %d" % MIN_BYTES, "free 1", "alloc 2 %d" % MIN_BYTES, "free 2", "close"]
    m = clean(run(programs, s, ARENA_MB=0))
    assert [e[0] for e in m.ops[2].events] == ["free"] and m.ops[2].st["cached"] == 0
    assert [e[0] for e in m.ops[4].events] == ["sync"] and m.ops[4].st["cached"] == MIN_BYTES
    assert m.ops[5].events == [] and m.ops[5].res == m.ops[3].res and [k for _, k in m.handouts] == ["direct", "direct", "kept"]


def test_best_fit_wastes_a_quarter_at_most(programs):
    """a kept block of exactly 1.25 x the request is handed out whole; one granule more and the request is carved out of it"""
    n = 160 * MiB
    s = ["open", "alloc 0 %d" % (n + n // 4), "free 0", "alloc 1 %d" % n, "free 1", "trim",
         "alloc 2 %d" % (n + n // 4 + GRANULE), "free 2", "alloc 3 %d" % n, "alloc 4 %d" % (n // 4), "free 3", "free 4", "close"]
    m = clean(run(programs, s))
    assert [k for _, k in m.handouts] == ["direct", "kept", "direct", "carved", "carved"]   # (40 MiB fit the rest of a block below one arena)
    assert m.ops[3].res == m.ops[1].res and m.ops[8].res == m.ops[6].res
    assert m.ops[11].st["cached"] == n + n // 4 + GRANULE   # (rule 5: the carved block is a kept block again)


def test_last_piece_of_an_arena_comes_back_inside_a_defer(programs):
    """rule 2 where an arena starts over: its pieces wait for the end of the Defer, nothing is placed over them before"""
    s = ["open", "alloc 0 5000", "alloc 1 70000", "defer+", "free 0", "free 1", "alloc 2 5000", "alloc 3 70000", "defer-",
         "alloc 4 5000", "free 2", "free 3", "free 4", "close"]
    m = clean(run(programs, s))
    assert m.ops[4].events == [] and m.ops[5].events == [] and m.ops[5].st["pending"] == 2
    assert m.ops[8].events == [("sync", 0)] and m.ops[9].res in (m.ops[1].res, m.ops[2].res)   # (handed out again after the sync)


def test_reuse_of_an_arena_piece_counts_as_use(programs):
    """a piece handed out again from the kept pieces keeps its arena from starting over under it"""
    s = ["open", "alloc 0 5000", "alloc 1 6000", "free 0", "alloc 2 5000", "free 1", "alloc 3 5000", "alloc 4 6000",
         "free 2", "free 3", "free 4", "close"]
    m = clean(run(programs, s))
    assert m.ops[4].res == m.ops[1].res


def test_small_buffers_do_not_pin_large_blocks(programs):
    """rule 7 both ways: a small request neither turns a kept 1 GB block into an arena, nor moves into the room a large request
    left in one"""
    s = ["open", "alloc 0 %d" % GB, "free 0", "alloc 1 256", "alloc 2 %d" % (600 * 10 ** 6), "alloc 3 256", "alloc 4 %d" % (90 * MiB),
         "free 2", "alloc 5 %d" % (80 * MiB)] + ["free %d" % i for i in (1, 3, 4, 5)] + ["close"]
    m = clean(run(programs, s))
    assert [k for _, k in m.handouts] == ["direct", "fresh arena", "carved", "arena", "arena", "arena"]
    assert m.ops[8].st["cached"] == GB


def test_refused_requests_and_reclaim(programs):
    """rule 6 on a card of 2 GB: a request that fits only without the kept block gets it after the trim; one that does not fit is
    refused, leaves hipGetLastError empty and the pool intact"""
    s = ["open", "cap 0 %d" % (2 * GB), "alloc 0 %d" % (1500 * 10 ** 6), "free 0", "alloc 1 %d" % (1900 * 10 ** 6), "alloc 2 %d" % (500 * 10 ** 6),
         "alloc 3 1000", "alloc 4 %d" % (99 * 10 ** 6), "free 1", "alloc 5 1000", "free 4", "free 5", "free 3", "close"]
    m = clean(run(programs, s))
    assert [op.res == "err" for op in m.ops[4:8]] == [False, True, False, False]
    assert [e[0] for e in m.ops[4].events] == ["free", "malloc"]
    assert [k for _, k in m.handouts] == ["direct"] * 5   # (small requests go to the driver on their own where no arena fits the card)


def test_blocks_come_back_while_another_device_is_current(programs):
    """rule 8: the synchronisation is of the device the block belongs to, at once and at the end of a Defer, the block returns to
    that device's requests only, and the caller's device stays current"""
    big = 200 * MiB
    s = ["open", "dev 0", "alloc 0 5000", "alloc 1 %d" % big, "dev 1", "alloc 2 5000", "alloc 3 %d" % big, "free 0", "free 1",
         "alloc 4 %d" % big, "dev 0", "alloc 5 %d" % big, "defer+", "free 2", "free 3", "free 4", "dev 1", "free 5", "defer-",
         "alloc 6 %d" % big, "alloc 7 5000", "dev 0", "alloc 8 %d" % big, "free 6", "free 7", "free 8", "close"]
    m = clean(run(programs, s))
    assert m.ops[7].events == [("sync", 0)] and m.ops[8].events == [("sync", 0)]
    assert m.ops[9].count("malloc") == 1 and m.ops[11].res == m.ops[3].res
    assert sorted(m.ops[18].events) == [("sync", 0), ("sync", 1)]
    assert m.ops[19].count("malloc") == 0 and m.ops[22].res == m.ops[3].res


def test_nothing_stays_behind_the_last_context(programs):
    """rule 4 on the paths where the order is unusual: the last context closes inside a Defer with blocks waiting, and a block
    comes back after the last context is gone"""
    s = ["open", "defer+", "alloc 0 5000", "alloc 1 %d" % (200 * MiB), "free 0", "free 1", "close", "defer-",
         "open", "alloc 2 5000", "alloc 3 %d" % (200 * MiB), "close", "free 2", "free 3"]
    m = clean(run(programs, s))
    assert m.ops[7].st["out"] == 0 and m.ops[-1].st["out"] == 0
    assert all(v == 0 for k, v in m.ops[-1].st.items() if k not in ("dev", "lasterr"))


def test_the_model_notices_a_broken_trace(programs):
    """the judge itself: the same trace with one event taken out, or one address moved, breaks the rule it should"""
    s = ["open", "alloc 0 5000", "alloc 1 %d" % (200 * MiB), "free 1", "alloc 2 %d" % (200 * MiB), "free 0", "free 2", "close"]
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    text = subprocess.run([programs["asan"]], input="\n".join(s) + "\n", stdout=subprocess.PIPE, universal_newlines=True, env=env, check=True).stdout
    assert not pool_model.replay(text).violations
    lines = text.splitlines()
    sync = [i for i, line in enumerate(lines) if line == "ev sync 0"]
    assert 2 in {v[0] for v in pool_model.replay("\n".join(lines[:sync[0]] + lines[sync[0] + 1:])).violations}
    small = pool_model.parse(text)[1][1].res
    big = pool_model.parse(text)[1][2].res
    shifted = "\n".join(line.replace("res ok %d" % small, "res ok %d" % (big + 4096)) for line in lines)
    assert 1 in {v[0] for v in pool_model.replay(shifted).violations}
    leaked = "\n".join(line for line in lines if not line.startswith("ev free"))
    assert {4, 5} & {v[0] for v in pool_model.replay(leaked).violations}


# ------------------------------------------------------------------ threads

@pytest.mark.parametrize("seed", [1, 2])
def test_threads_under_the_thread_sanitizer(programs, seed):
    """eight threads allocate and free while one of them opens and closes Defer objects: no report of the sanitizer, no two blocks
    in use overlap, nothing waits after the last Defer, nothing is at the driver after the last context (the program checks)"""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(FEMSHELL_POOL_GB="2", FEMSHELL_POOL_ARENA_MB="192")
    r = subprocess.run([programs["tsan"], "threads", "8", str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stderr == "" and r.stdout.strip() == "threads ok", r.stdout[-500:] + r.stderr[-3000:]


# ------------------------------------------------------------------ the counters' way out of the library

def test_pool_stats_is_declared_exported_and_bound():
    import ctypes
    import re
    from importlib import import_module

    from tests.helpers.product import ensure_built

    pkg = ensure_built()
    with open(os.path.join(ROOT, "include", "femshell.h")) as f:
        assert re.search(r"\bint\s+femshell_pool_stats\s*\(\s*double out\[6\]\s*\)", f.read())
    assert hasattr(ctypes.CDLL(pkg.library_path()), "femshell_pool_stats")
    binding = import_module("fem-shell_amd.binding")
    assert "femshell_pool_stats" in binding.SYMBOLS and pkg.load_library().femshell_pool_stats.argtypes is not None
    assert callable(pkg.pool_stats)
