#!/usr/bin/env python3
"""The elastic supports on the 4M-triangle panel (one MI355X), beside the assembly in the same run.

On one context: the medians of femshell_time_kernel for KERNEL_ELASTIC_SUPPORT (k_support_rows: a workgroup per slice, the six
words of B_e through LDS) and KERNEL_ASSEMBLE, and of the event-timed femshell_assemble with the supports in force and without
(the difference is k_support_add, a lane per node behind the assembly kernel), alternating `rounds` times.  Beside them the
assembly time the parent commit recorded on the same mesh (profiles/element_loads_panel4m.txt).  No threshold: the kernels run
once per change of the supports, not per iteration, and nothing on the timed path of bench.py runs them.

    python tools/elastic_support_profile.py [--n 1414] [--rounds 7] [--reps 5]
"""
import argparse
import importlib
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parent_assemble_ms():
    """the median the parent commit recorded for the assembly kernel on this mesh, or None"""
    try:
        text = open(os.path.join(ROOT, "profiles", "element_loads_panel4m.txt")).read()
    except OSError:
        return None
    found = re.search(r"^assemble\s+median ([0-9.]+) ms", text, re.M)
    return float(found.group(1)) if found else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1414, help="squares per side of the panel (1414: 4M triangles)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "elastic_support_panel4m.txt"))
    args = ap.parse_args()
    from tests.helpers import fullsize

    pkg = importlib.import_module("fem-shell_amd")
    binding = importlib.import_module("fem-shell_amd.binding")
    m, (nu, E, t) = fullsize.workload("panel", args.n)
    fs = pkg.FemShell(nu, E, t, device=0)
    fs.set_mesh(m.xyz, m.tri, m.quad)
    fs.set_dirichlet(m.dirichlet_mask())
    fs.set_loads(m.loads)
    tk = np.tile([1e4, 1e2], (len(m.tri), 1))
    springs = np.zeros((m.n_nodes, 6))
    springs[::3] = [2e3, 1e3, 3e3, 40.0, 50.0, 60.0]
    kernels = (("support_rows", binding.KERNEL_ELASTIC_SUPPORT), ("assemble", binding.KERNEL_ASSEMBLE))
    samples = {k: [] for k, _ in kernels}
    samples["assemble call, supports"] = []
    samples["assemble call, none"] = []
    nbytes = {}

    def assemble_ms():
        """one femshell_assemble by its event pair, as the next solve reports it"""
        fs.set_dirichlet(m.dirichlet_mask())  # (makes K stale)
        return 1e3 * fs.solve(rtol=1e-2, max_it=1, fetch=False)[1]["assemble_seconds"]

    for r in range(args.rounds + 1):  # (round 0 warms up: first-use costs of the kernels)
        for name, which in kernels:
            ms, nbytes[name] = fs.time_kernel(which, reps=args.reps)
            if r:
                samples[name].append(ms)
        fs.set_foundation(tk)
        fs.set_springs(springs)
        with_supports = assemble_ms()
        fs.set_foundation(None, None)
        fs.set_springs(None)
        without = assemble_ms()
        if r:
            samples["assemble call, supports"].append(with_supports)
            samples["assemble call, none"].append(without)
    med = {k: float(np.median(v)) for k, v in samples.items()}
    lines = ["# panel %d x %d squares: %d tri3, %d nodes" % (args.n, args.n, len(m.tri), m.n_nodes),
             "# medians of %d alternating rounds; kernels: %d launches each, back to back, ms per launch; calls: one event-timed assembly" % (args.rounds, args.reps)]
    for name in samples:
        line = "%-26s median %.4f ms  (min %.4f, max %.4f)" % (name, med[name], min(samples[name]), max(samples[name]))
        if name in nbytes:
            line += "  algorithmic bytes %.4e  %.3f TB/s" % (nbytes[name], nbytes[name] / (med[name] * 1e-3) / 1e12)
        lines.append(line)
    lines.append("k_support_add (assemble call with supports - without) = %.4f ms" % (med["assemble call, supports"] - med["assemble call, none"]))
    lines.append("support_rows / assemble = %.3f" % (med["support_rows"] / med["assemble"]))
    parent = parent_assemble_ms()
    lines.append("assemble of the parent commit (profiles/element_loads_panel4m.txt): %s" % ("%.4f ms" % parent if parent else "not recorded"))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f_out:
        f_out.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    fs.close()


if __name__ == "__main__":
    main()
