#!/usr/bin/env python3
"""Load cases against as many single solves (one MI355X, block-Jacobi), on one context each of the 4M-triangle panel and of a
20k-node panel.

For 1, 2, 4 and 8 cases at a fixed iteration count (rtol = 0): femshell_solve_cases in one call, and femshell_set_loads +
femshell_solve once per case -- the path a caller had before -- alternating in one process, `rounds` times behind a warm-up round.
Reported: the medians of the device seconds per iteration (solve_seconds of the two info structures: the Krylov loops, without
transfers and assembly), their ratio, and the algorithmic bytes per iteration of each.  Writes profiles/load_cases_ab.txt.

    python tools/cases_profile.py [--sizes 1414,141] [--rounds 3] [--iterations 20,200]
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
    ap.add_argument("--sizes", default="1414,141", help="squares per side of the panels (1414: 4M triangles, 141: 20k nodes)")
    ap.add_argument("--iterations", default="20,200", help="iterations per solve, one number per size")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", default="1,2,4,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "load_cases_ab.txt"))
    args = ap.parse_args()
    from tests.helpers import fullsize

    pkg = importlib.import_module("fem-shell_amd")
    sizes = [int(v) for v in args.sizes.split(",")]
    iterations = [int(v) for v in args.iterations.split(",")]
    counts = [int(v) for v in args.cases.split(",")]
    lines = ["# femshell_solve_cases against n x (femshell_set_loads + femshell_solve), block-Jacobi, rtol = 0: device seconds per iteration",
             "# medians of %d alternating rounds behind a warm-up round" % args.rounds]
    for n, K in zip(sizes, iterations):
        m, (nu, E, t) = fullsize.workload("panel", n)
        fs = pkg.FemShell(nu, E, t, device=0)
        fs.set_mesh(m.xyz, m.tri, m.quad)
        fs.set_dirichlet(m.dirichlet_mask())
        fs.set_loads(m.loads)
        fs.set_preconditioner("jacobi")
        fs.assemble()
        lines.append("# panel %d x %d squares: %d tri3, %d nodes, %d iterations per solve" % (n, n, len(m.tri), m.n_nodes, K))
        rng = np.random.default_rng(3)
        L = np.stack([m.loads.reshape(-1, 6) * (1.0 + j) + rng.uniform(-1e-3, 1e-3, (m.n_nodes, 6)) for j in range(max(counts))])
        for nc in counts:
            together, single = [], []
            bytes_together = bytes_single = 0.0
            for r in range(args.rounds + 1):
                _, cases, info = fs.solve_cases(L[:nc], rtol=0.0, max_it=K)
                assert all(c["iterations"] == K for c in cases), cases
                a = info["solve_seconds"] / K
                bytes_together = info["bytes_per_iteration"]
                b = 0.0
                bytes_single = 0.0
                for j in range(nc):
                    fs.set_loads(L[j])
                    _, si = fs.solve(rtol=0.0, max_it=K, fetch=False)
                    assert si["iterations"] == K, si
                    b += si["solve_seconds"] / K
                    bytes_single += si["bytes_per_iteration"]
                if r:
                    together.append(a)
                    single.append(b)
            ta, tb = float(np.median(together)), float(np.median(single))
            lines.append("%8d nodes  %d cases  solve_cases %.4e s/iteration (%.3e B, %.2f TB/s)   %d x solve %.4e s/iteration (%.3e B, %.2f TB/s)   ratio %.2f  passes %d fused %d"
                         % (m.n_nodes, nc, ta, bytes_together, bytes_together / ta / 1e12, nc, tb, bytes_single, bytes_single / tb / 1e12, tb / ta,
                            info["passes"], info["fused_product"]))
            print(lines[-1], flush=True)
        fs.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
