#!/usr/bin/env python3
"""Modal analysis on the 4M-triangle panel (one MI355X).

(a) The fused block product against the existing single-vector kernels, on one context: femshell_time_kernel(KERNEL_SPMM) for 4
    and 8 columns with the fused kernel and -- FEMSHELL_SPMM_FUSED=0 -- column by column through launch_spmv (both phases of the
    symmetric product each), and the same number of KERNEL_SPMV launches as the library times them (inside the CG recurrence,
    first phase only: the update kernel collects the transposed products there).  The variants alternate, `rounds` times; the
    medians are reported with the algorithmic bytes of each.  Writes profiles/modal_product_ab.txt.
(b) One femshell_modes(n_modes = 8) run: iterations and the split of its seconds.  Writes profiles/modal_panel4m.json.

    python tools/modal_profile.py [--n 1414] [--rounds 5] [--reps 5] [--skip-modes]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1414, help="squares per side of the panel (1414: 4M triangles)")
    ap.add_argument("--rho", type=float, default=7.8e-3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-modes", type=int, default=8)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--max-it", type=int, default=200)
    ap.add_argument("--skip-modes", action="store_true")
    ap.add_argument("--out-ab", default=os.path.join(ROOT, "profiles", "modal_product_ab.txt"))
    ap.add_argument("--out-modes", default=os.path.join(ROOT, "profiles", "modal_panel4m.json"))
    args = ap.parse_args()
    from tests.helpers import fullsize

    pkg = importlib.import_module("fem-shell_amd")
    binding = importlib.import_module("fem-shell_amd.binding")
    m, (nu, E, t) = fullsize.workload("panel", args.n)
    fs = pkg.FemShell(nu, E, t, device=0)
    fs.set_mesh(m.xyz, m.tri, m.quad)
    fs.set_dirichlet(m.dirichlet_mask())
    fs.set_loads(m.loads)
    fs.set_preconditioner("amg")
    fs.set_density(args.rho)
    fs.assemble()
    mesh = "panel %d x %d squares: %d tri3, %d nodes" % (args.n, args.n, len(m.tri), m.n_nodes)

    lines = ["# " + mesh, "# medians of %d alternating rounds, %d launches each; ms per block product" % (args.rounds, args.reps)]
    for cols in (4, 8):
        os.environ["FEMSHELL_TIME_KERNEL_COLS"] = str(cols)
        samples = {"fused": [], "columnwise": [], "spmv_phase1_x_cols": []}
        bytes_of = {}
        for r in range(args.rounds + 1):  # (round 0 warms up: first-use costs of the kernels)
            os.environ["FEMSHELL_SPMM_FUSED"] = "1"
            ms, bytes_of["fused"] = fs.time_kernel(binding.KERNEL_SPMM, reps=args.reps)
            a = ms
            os.environ["FEMSHELL_SPMM_FUSED"] = "0"
            ms, bytes_of["columnwise"] = fs.time_kernel(binding.KERNEL_SPMM, reps=args.reps)
            b = ms
            ms, by = fs.time_kernel(binding.KERNEL_SPMV, reps=args.reps)
            bytes_of["spmv_phase1_x_cols"] = cols * by
            if r:
                samples["fused"].append(a)
                samples["columnwise"].append(b)
                samples["spmv_phase1_x_cols"].append(cols * ms)
        os.environ["FEMSHELL_SPMM_FUSED"] = "1"
        med = {k: float(np.median(v)) for k, v in samples.items()}
        for k in ("fused", "columnwise", "spmv_phase1_x_cols"):
            lines.append("%d columns  %-20s median %.4f ms  (min %.4f, max %.4f)  algorithmic bytes %.4e  %.3f TB/s" % (
                cols, k, med[k], min(samples[k]), max(samples[k]), bytes_of[k], bytes_of[k] / (med[k] * 1e-3) / 1e12))
        lines.append("%d columns  column by column / fused = %.3f   %d x spmv (first phase) / fused = %.3f" % (
            cols, med["columnwise"] / med["fused"], cols, med["spmv_phase1_x_cols"] / med["fused"]))
    os.makedirs(os.path.dirname(args.out_ab), exist_ok=True)
    with open(args.out_ab, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))

    if not args.skip_modes:
        lam, _, res, info = fs.modes(args.n_modes, tol=args.tol, max_it=args.max_it, want_modes=False)
        result = {"mesh": mesh, "n_modes": args.n_modes, "tol": args.tol, "max_it": args.max_it, "rho": args.rho,
                  "lambda": [float(x) for x in lam], "residual": [float(x) for x in res], "info": info}
        with open(args.out_modes, "w") as f:
            json.dump(result, f, indent=1)
        print(json.dumps(result))
    fs.close()


if __name__ == "__main__":
    main()
