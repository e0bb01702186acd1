#!/usr/bin/env python3
"""Cost of a Newmark step on the 4M-triangle panel (one MI355X): milliseconds and algorithmic bytes of k_lumped_mass,
k_mass_shift, k_newmark_rhs and k_newmark_update (femshell_time_kernel: HIP events around back-to-back launches), and
the iterations and seconds of a step's solve beside the static solve of the same system (multigrid, rtol 1e-10).

dt = T1 / 20 with T1 from a few steps of inverse iteration x <- K^-1 M x on the device (Rayleigh quotient x.Kx / x.Mx).
Writes profiles/dynamics_step.json; DESIGN.md quotes it.

    python tools/dynamics_profile.py [--n 1414] [--steps 5] [--out profiles/dynamics_step.json]
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
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rho", type=float, default=7.8e-3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dynamics_step.json"))
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
    rtol, max_it = 1e-10, 3000
    fs.solve(rtol=rtol, max_it=max_it, fetch=False)  # (assembly, hierarchy, first-use costs)
    u, static = fs.solve(rtol=rtol, max_it=max_it)
    mass = fs.lumped_mass()
    # inverse iteration for the first period: x <- K^-1 M x, omega^2 = x.Kx / x.Mx = x.(M x_prev) / x.Mx
    x, w2 = u, None
    history = []
    for _ in range(4):
        b = mass * x
        fs.set_loads(b)
        x, _ = fs.solve(rtol=rtol, max_it=max_it)
        w2 = float((x * b).sum() / (x * mass * x).sum())
        history.append(w2)
        x = x / np.abs(x).max()
    T1 = 2.0 * np.pi / np.sqrt(w2)
    dt = T1 / 20.0
    # free vibration from the static deflection with the load removed
    fs.set_loads(np.zeros_like(m.loads))
    fs.dynamics_begin(dt, u0=u)
    steps = []
    for _ in range(args.steps):
        info = fs.dynamics_step(rtol=rtol, max_it=max_it)
        fs.dynamics_accept()
        steps.append({k: info[k] for k in ("iterations", "converged", "solve_seconds", "pc_setup_seconds", "setup_seconds",
                                           "assemble_seconds", "bytes_per_iteration", "amg_levels")})
    energy = fs.dynamics_energy()
    kernels = {}
    for name, which in (("k_newmark_rhs", binding.KERNEL_NEWMARK_RHS), ("k_newmark_update", binding.KERNEL_NEWMARK_UPDATE),
                        ("k_lumped_mass", binding.KERNEL_LUMPED_MASS), ("k_mass_shift", binding.KERNEL_MASS_SHIFT)):
        ms, by = fs.time_kernel(which, reps=args.reps)
        kernels[name] = {"ms": ms, "algorithmic_bytes": by, "TB_per_s": by / (ms * 1e-3) / 1e12}
    per_step_ms = kernels["k_newmark_rhs"]["ms"] + kernels["k_newmark_update"]["ms"]
    later = steps[1:] if len(steps) > 1 else steps
    solve_ms = 1e3 * float(np.mean([s["solve_seconds"] for s in later]))
    result = {
        "mesh": "panel %d x %d squares: %d tri3, %d nodes" % (args.n, args.n, len(m.tri), m.n_nodes),
        "rtol": rtol, "rho": args.rho, "T1": T1, "dt": dt, "omega2_by_inverse_iteration": history,
        "static_solve": {k: static[k] for k in ("iterations", "converged", "solve_seconds", "bytes_per_iteration", "amg_levels")},
        "steps": steps, "kernels": kernels,
        "step_kernels_ms": per_step_ms, "step_solve_ms_mean_after_the_first": solve_ms,
        "step_kernels_over_solve": per_step_ms / solve_ms,
        "energy_after_the_steps": {"kinetic": energy[0], "strain": energy[1]},
    }
    fs.dynamics_end()
    fs.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
