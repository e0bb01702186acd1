#!/usr/bin/env python3
"""The geometric product on the 4M-triangle panel (one MI355X), beside the block product with K and the element loads in the
same run.

On one context: the medians of femshell_time_kernel for KERNEL_GEOMETRIC_PRODUCT (k_geometric_product: one pass of four columns,
a workgroup per slice, the entries' products through LDS), KERNEL_SPMM (k_spmm_sym: Y = K X for four columns over the stored
blocks) and KERNEL_ELEMENT_LOADS (k_element_loads: the same walk over the slices' element lists with one vector), the three
alternating `rounds` times, with the algorithmic bytes of each.  No threshold: nothing on the timed path of bench.py runs the
kernel.

    python tools/geometric_product_profile.py [--n 1414] [--rounds 7] [--reps 5]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geometric_product_panel4m.txt"))
    args = ap.parse_args()
    from tests.helpers import fullsize

    pkg = importlib.import_module("fem-shell_amd")
    binding = importlib.import_module("fem-shell_amd.binding")
    m, (nu, E, t) = fullsize.workload("panel", args.n)
    fs = pkg.FemShell(nu, E, t, device=0)
    fs.set_mesh(m.xyz, m.tri, m.quad)
    fs.set_dirichlet(m.dirichlet_mask())
    fs.assemble()  # (the block product needs K)
    kernels = (("geometric_product", binding.KERNEL_GEOMETRIC_PRODUCT), ("spmm", binding.KERNEL_SPMM), ("element_loads", binding.KERNEL_ELEMENT_LOADS))
    samples = {k: [] for k, _ in kernels}
    nbytes = {}
    for r in range(args.rounds + 1):  # (round 0 warms up: first-use costs of the kernels)
        for name, which in kernels:
            ms, nbytes[name] = fs.time_kernel(which, reps=args.reps)
            if r:
                samples[name].append(ms)
    med = {k: float(np.median(v)) for k, v in samples.items()}
    lines = ["# panel %d x %d squares: %d tri3, %d nodes" % (args.n, args.n, len(m.tri), m.n_nodes),
             "# medians of %d alternating rounds, %d launches each, back to back; ms per launch; geometric_product and spmm: four columns" % (args.rounds, args.reps)]
    for name, _ in kernels:
        lines.append("%-20s median %.4f ms  (min %.4f, max %.4f)  algorithmic bytes %.4e  %.3f TB/s"
                     % (name, med[name], min(samples[name]), max(samples[name]), nbytes[name], nbytes[name] / (med[name] * 1e-3) / 1e12))
    lines.append("geometric_product / spmm = %.3f, geometric_product / element_loads = %.3f"
                 % (med["geometric_product"] / med["spmm"], med["geometric_product"] / med["element_loads"]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f_out:
        f_out.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    fs.close()


if __name__ == "__main__":
    main()
