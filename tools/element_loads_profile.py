#!/usr/bin/env python3
"""The element loads on the 4M-triangle panel (one MI355X), beside the lumped mass and the assembly in the same run.

On one context: the medians of femshell_time_kernel for KERNEL_ELEMENT_LOADS (k_element_loads: a workgroup per slice, share
vectors through LDS), KERNEL_LUMPED_MASS (k_lumped_mass: the lane-per-row walk over the same lists) and KERNEL_ASSEMBLE, the three
alternating `rounds` times, with the algorithmic bytes of each.  Beside them the wall time of one set_element_loads call (host
permutation, 32 bytes per element to HBM, one launch) and of the path it replaces: lumping the pressure to nodes in numpy and
set_loads of the dense vector.  No threshold: nothing on the timed path of bench.py runs the kernel.

    python tools/element_loads_profile.py [--n 1414] [--rounds 7] [--reps 5]
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def lump_in_numpy(xyz, tri, p):
    """the caller's side of a uniform pressure without the library: p (b-a) x (c-a) / 6 to each node of every triangle"""
    a, b, c = xyz[tri[:, 0]], xyz[tri[:, 1]], xyz[tri[:, 2]]
    share = np.cross(b - a, c - a) * (p / 6.0)
    f = np.zeros((len(xyz), 6))
    for d in range(3):
        f[:, d] = np.bincount(tri.ravel(), weights=np.repeat(share[:, d], 3), minlength=len(xyz))
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1414, help="squares per side of the panel (1414: 4M triangles)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "element_loads_panel4m.txt"))
    args = ap.parse_args()
    from tests.helpers import fullsize

    pkg = importlib.import_module("fem-shell_amd")
    binding = importlib.import_module("fem-shell_amd.binding")
    m, (nu, E, t) = fullsize.workload("panel", args.n)
    fs = pkg.FemShell(nu, E, t, device=0)
    fs.set_mesh(m.xyz, m.tri, m.quad)
    fs.set_dirichlet(m.dirichlet_mask())
    fs.set_density(7.8e-3)  # (the lumped mass needs one)
    kernels = (("element_loads", binding.KERNEL_ELEMENT_LOADS), ("lumped_mass", binding.KERNEL_LUMPED_MASS), ("assemble", binding.KERNEL_ASSEMBLE))
    samples = {k: [] for k, _ in kernels}
    nbytes = {}
    for r in range(args.rounds + 1):  # (round 0 warms up: first-use costs of the kernels)
        for name, which in kernels:
            ms, nbytes[name] = fs.time_kernel(which, reps=args.reps)
            if r:
                samples[name].append(ms)
    med = {k: float(np.median(v)) for k, v in samples.items()}
    # the calls: the median of `rounds` of each, after one of each that is not counted
    tl = np.zeros((len(m.tri), 4))
    tl[:, 0] = 300.0
    wall = {"set_element_loads": [], "numpy lumping": [], "set_loads (dense)": []}
    fs.set_element_loads(tl)
    for r in range(args.rounds + 1):
        t0 = time.perf_counter()
        fs.set_element_loads(tl)  # (a set that replaces one in force: the call of a coupled loop)
        fs.sync()
        t1 = time.perf_counter()
        fs.set_element_loads(None, None)  # (not timed: the path that is replaced runs without element loads)
        fs.sync()
        t2 = time.perf_counter()
        f = lump_in_numpy(m.xyz, m.tri, 300.0)
        t3 = time.perf_counter()
        fs.set_loads(f)
        fs.sync()
        t4 = time.perf_counter()
        fs.set_element_loads(tl)
        if r:
            wall["set_element_loads"].append(t1 - t0)
            wall["numpy lumping"].append(t3 - t2)
            wall["set_loads (dense)"].append(t4 - t3)
    S = fs.element_load_vector()
    agree = float(np.abs(S - f).max() / np.abs(f).max())
    lines = ["# panel %d x %d squares: %d tri3, %d nodes" % (args.n, args.n, len(m.tri), m.n_nodes),
             "# medians of %d alternating rounds, %d launches each, back to back; ms per launch" % (args.rounds, args.reps)]
    for name, _ in kernels:
        lines.append("%-20s median %.4f ms  (min %.4f, max %.4f)  algorithmic bytes %.4e  %.3f TB/s"
                     % (name, med[name], min(samples[name]), max(samples[name]), nbytes[name], nbytes[name] / (med[name] * 1e-3) / 1e12))
    lines.append("element_loads / lumped_mass = %.3f, element_loads / assemble = %.3f"
                 % (med["element_loads"] / med["lumped_mass"], med["element_loads"] / med["assemble"]))
    lines.append("# wall time of the calls, uniform pressure 300, medians of %d; set_element_loads replaces a set in force" % args.rounds)
    for name, v in wall.items():
        lines.append("%-20s median %.2f ms  (min %.2f, max %.2f)" % (name, 1e3 * np.median(v), 1e3 * min(v), 1e3 * max(v)))
    lines.append("max |S - numpy lumping| / max |numpy lumping| = %.2e" % agree)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f_out:
        f_out.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    fs.close()


if __name__ == "__main__":
    main()
