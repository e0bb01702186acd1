#!/usr/bin/env python3
"""The thermal loads on the 4M-triangle panel (one MI355X), beside the element loads in the same run.

On one context: the medians of femshell_time_kernel for KERNEL_ELEMENT_THERMAL (k_element_thermal: a workgroup per slice, the
elements' per-node 6-vectors through LDS) and KERNEL_ELEMENT_LOADS (k_element_loads, the yardstick: the same walk with one share
vector per element), alternating `rounds` times, with the algorithmic bytes of each and the fraction of 8 TB/s they reach.  Beside
them the wall time of one set_thermal call that replaces a set in force (host permutation, 16 bytes per element to HBM, one
launch).  No threshold: nothing on the timed path of bench.py runs the kernel.

    python tools/thermal_profile.py [--n 1414] [--rounds 7] [--reps 5]
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12  # bytes per second of HBM the fractions are taken of


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1414, help="squares per side of the panel (1414: 4M triangles)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thermal_panel4m.txt"))
    args = ap.parse_args()
    from tests.helpers import fullsize

    pkg = importlib.import_module("fem-shell_amd")
    binding = importlib.import_module("fem-shell_amd.binding")
    m, (nu, E, t) = fullsize.workload("panel", args.n)
    fs = pkg.FemShell(nu, E, t, device=0)
    fs.set_mesh(m.xyz, m.tri, m.quad)
    fs.set_dirichlet(m.dirichlet_mask())
    kernels = (("element_thermal", binding.KERNEL_ELEMENT_THERMAL), ("element_loads", binding.KERNEL_ELEMENT_LOADS))
    samples = {k: [] for k, _ in kernels}
    nbytes = {}
    for r in range(args.rounds + 1):  # (round 0 warms up: first-use costs of the kernels)
        for name, which in kernels:
            ms, nbytes[name] = fs.time_kernel(which, reps=args.reps)
            if r:
                samples[name].append(ms)
    med = {k: float(np.median(v)) for k, v in samples.items()}
    temps = np.tile([40.0, -15.0], (len(m.tri), 1))
    fs.set_expansion(1.2e-5)
    fs.set_thermal(temps)
    wall = []
    for r in range(args.rounds + 1):
        t0 = time.perf_counter()
        fs.set_thermal(temps)  # (a set that replaces one in force: the call of a coupled loop)
        fs.sync()
        if r:
            wall.append(time.perf_counter() - t0)
    lines = ["# panel %d x %d squares: %d tri3, %d nodes" % (args.n, args.n, len(m.tri), m.n_nodes),
             "# medians of %d alternating rounds, %d launches each, back to back; ms per launch" % (args.rounds, args.reps)]
    for name, _ in kernels:
        rate = nbytes[name] / (med[name] * 1e-3)
        lines.append("%-20s median %.4f ms  (min %.4f, max %.4f)  algorithmic bytes %.4e  %.3f TB/s  %.3f of 8 TB/s"
                     % (name, med[name], min(samples[name]), max(samples[name]), nbytes[name], rate / 1e12, rate / PEAK))
    lines.append("element_thermal / element_loads = %.3f in time, %.3f in time per algorithmic byte"
                 % (med["element_thermal"] / med["element_loads"],
                    (med["element_thermal"] / nbytes["element_thermal"]) / (med["element_loads"] / nbytes["element_loads"])))
    lines.append("# wall time of the call, uniform (Tm, Tg) = (40, -15), median of %d; set_thermal replaces a set in force" % args.rounds)
    lines.append("%-20s median %.2f ms  (min %.2f, max %.2f)" % ("set_thermal", 1e3 * float(np.median(wall)), 1e3 * min(wall), 1e3 * max(wall)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "w") as f:
        f.write(text)
    fs.close()


if __name__ == "__main__":
    main()
