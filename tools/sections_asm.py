"""Cost of shell sections in the assembly kernel (femshell_time_kernel, FEMSHELL_KERNEL_ASSEMBLE), against the same context
without sections: (a) uniform, (b) three strips, (c) one section per element -- on the NX^2 triangle panel (default 1414: 4.0 M
triangles) and, for (a) and (b), on a panel of QNX^2 quadrilaterals (default 2000: 4.0 M).  Also the wall time of
femshell_set_sections against femshell_set_mesh.  Prints one line per measurement.

    python tools/sections_asm.py            # NX=1414 QNX=2000 ASM_REPS=20
"""
import importlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("fem-shell_amd")
meshgen = importlib.import_module("fem-shell_amd.meshgen")

REPS = int(os.environ.get("ASM_REPS", "20"))
STRIPS = np.array([[0.3, 2e5, 0.05], [0.25, 7e4, 0.1], [0.33, 1e5, 0.025]])


_cold = [True]


def timed(fs, label, n_elem):
    # the first launches of a process run slow (clocks, TLBs; 0.67 against 0.59 ms measured here): warm up well once
    for _ in range(40 if _cold[0] else 3):
        fs.assemble()
    _cold[0] = False
    ms, by = fs.time_kernel(pkg.KERNEL_ASSEMBLE, REPS)
    print("%-44s %-16s %.3f ms  %.0f GB/s  %.2f G elements/s" % (label, fs.assembly_kernel(), ms, by / ms / 1e6, n_elem / ms / 1e6), flush=True)
    return ms


def strips_of(xyz, conn):
    cx = xyz[conn][:, :, 0].mean(axis=1)
    return np.minimum((3 * (cx - cx.min()) / (cx.max() - cx.min())).astype(np.int32), 2)


def run(kind, n):
    m = meshgen.structured(n, n, 0.0, 0.0, 10.0, 10.0, kind=kind, ul_lr=True, bcids=(0, 0, 0, 0), factor=300.0, loading=2)
    conn = m.tri if kind == "t" else m.quad
    name = "%d %s" % (len(conn), "triangles" if kind == "t" else "quadrilaterals")
    fs = pkg.FemShell(0.3, 1e7, 0.5)
    t0 = time.perf_counter()
    fs.set_mesh(m.xyz, m.tri, m.quad)
    t_mesh = time.perf_counter() - t0
    fs.set_dirichlet(m.dirichlet_mask())
    fs.set_loads(m.loads)
    base = timed(fs, name + ", (a) no sections", len(conn))
    sec = strips_of(m.xyz, conn)
    args = (sec, None) if kind == "t" else (None, sec)
    t0 = time.perf_counter()
    fs.set_sections(STRIPS, *args)
    t_sec = time.perf_counter() - t0
    print("%-44s femshell_set_mesh %.3f s, femshell_set_sections %.3f s (%.1f %%)" % (name, t_mesh, t_sec, 100.0 * t_sec / t_mesh), flush=True)
    b = timed(fs, name + ", (b) three strips", len(conn))
    print("%-44s (b) / (a) = %.3f" % (name, b / base))
    if kind == "t":
        t = 0.02 * (1.0 + 3.0 * np.arange(len(conn)) / (len(conn) - 1.0))
        fs.set_sections(np.stack([np.full(len(conn), 0.3), np.full(len(conn), 1e7), t], axis=1), np.arange(len(conn), dtype=np.int32))
        c = timed(fs, name + ", (c) one section per element", len(conn))
        print("%-44s (c) / (a) = %.3f" % (name, c / base))
    fs.set_sections(None)
    again = timed(fs, name + ", (a) again, sections cleared", len(conn))
    print("%-44s (a) again / (a) = %.3f" % (name, again / base))
    fs.close()


if __name__ == "__main__":
    run("t", int(os.environ.get("NX", "1414")))
    if os.environ.get("QNX", "2000") != "0":
        run("q", int(os.environ.get("QNX", "2000")))
