#!/usr/bin/env python3
"""The nodal recovery on the 4M-triangle panel (one MI355X), beside the element resultants in the same run.

On one context: the medians of femshell_time_kernel for KERNEL_NODAL_RECOVERY (k_nodal_recovery: the element tensors averaged to the
nodes over the slices' element lists), KERNEL_RECOVERY_ERROR (k_recovery_error: e2 and eta^2 per element) and
KERNEL_ELEMENT_RESULTANTS (k_element_resultants, which writes the rows the other two read), the three alternating `rounds` times,
with the algorithmic bytes of each.  No threshold: nothing on the timed path of bench.py runs these kernels.

    python tools/nodal_recovery_profile.py [--n 1414] [--rounds 7] [--reps 5]
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1414, help="squares per side of the panel (1414: 4M triangles)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nodal_recovery_panel4m.txt"))
    args = ap.parse_args()
    from tests.helpers import fullsize

    pkg = importlib.import_module("fem-shell_amd")
    binding = importlib.import_module("fem-shell_amd.binding")
    m, (nu, E, t) = fullsize.workload("panel", args.n)
    fs = pkg.FemShell(nu, E, t, device=0)
    fs.set_mesh(m.xyz, m.tri, m.quad)
    kernels = (("nodal_recovery", binding.KERNEL_NODAL_RECOVERY), ("recovery_error", binding.KERNEL_RECOVERY_ERROR),
               ("element_resultants", binding.KERNEL_ELEMENT_RESULTANTS))
    samples = {k: [] for k, _ in kernels}
    nbytes = {}
    for r in range(args.rounds + 1):  # (round 0 warms up: first-use costs of the kernels)
        for name, which in kernels:
            ms, nbytes[name] = fs.time_kernel(which, reps=args.reps)
            if r:
                samples[name].append(ms)
    med = {k: float(np.median(v)) for k, v in samples.items()}
    lines = ["# panel %d x %d squares: %d tri3, %d nodes" % (args.n, args.n, len(m.tri), m.n_nodes),
             "# medians of %d alternating rounds, %d launches each, back to back on the element rows of a hashed vector; ms per launch"
             % (args.rounds, args.reps)]
    for name, _ in kernels:
        lines.append("%-20s median %.4f ms  (min %.4f, max %.4f)  algorithmic bytes %.4e  %.3f TB/s"
                     % (name, med[name], min(samples[name]), max(samples[name]), nbytes[name], nbytes[name] / (med[name] * 1e-3) / 1e12))
    for name in ("nodal_recovery", "recovery_error"):
        lines.append("%s / element_resultants = %.3f" % (name, med[name] / med["element_resultants"]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    fs.close()


if __name__ == "__main__":
    main()
