#!/usr/bin/env python3
"""Prints, for every case and state of tests/test_gpu_residual_truth.py, the worst error of femshell_residual against the exact
residual over the budget of tests/helpers/residual_truth.py, row by row, and the same quantity for amg_oracle.residual_extended,
the long-double evaluation the older tests compare with; then the worst per kernel.  profiles/residual_truth_vs_exact.txt is the
output of this script on an MI355X.

    python tools/residual_truth_report.py            needs a GPU
    python tools/residual_truth_report.py --model    CPU only: the numpy restatement of the kernels' arithmetic in place of the
                                                     device, on the oracle's assembly of the same meshes"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.helpers import residual_cases as rc, residual_truth as rt  # noqa: E402
from tests.helpers.product import ensure_built, pkg  # noqa: E402


def kernel_of(name):
    return "k_residual_dd" if name.startswith("full-") or name.startswith("walk-full") else "k_residual_dd_sym"


def roof_iterate(model_only):
    """the converged iterate of the 32 x 32 roof, no refinement pass (model: the oracle's direct solve of the oracle's assembly)"""
    from tests.helpers import meshes, oracle

    m = meshes.scordelis_lo(32)
    if model_only:
        r, c, v, F = oracle.assemble(m.xyz, m.tri, m.quad, oracle.material(*m.material), m.dirichlet_mask(), m.loads)
        u = oracle.direct_solve(r, c, v, F)
        res = rt.model((r, c, v), F, u, order="sym")
    else:
        fs = pkg.FemShell(*m.material, device=0)
        fs.set_mesh(m.xyz, m.tri, m.quad)
        fs.set_dirichlet(m.dirichlet_mask())
        fs.set_loads(m.loads)
        fs.set_preconditioner("amg", refine_passes=0)
        u, info = fs.solve(rtol=1e-12, max_it=500)
        assert info["converged"] == 1, info
        r, c, v, F = fs.export_bsr()
        res = fs.residual(u)
        fs.close()
        u = u.ravel()
    from oracle import amg_oracle

    K = (r, c, v)
    truth = rt.exact(K, F, u)
    budget = rt.bound(K, F, u, truth)
    ext = amg_oracle.residual_extended(rt.csr(K), F, u)
    return dict(ratio=float(rt.ratios(res, truth, budget).max()), ext=float(rt.ratios(ext, truth, budget).max()),
                cancel=rt.cancellation(truth, rt.scale(K, F, u)))


def main():
    model_only = "--model" in sys.argv[1:]
    if not model_only:
        ensure_built()
    print("femshell_residual against the exact residual, worst over the scalar rows of error / budget; budget per row "
          "u |r*| + gamma_m^2 (|F| + |K||x|), m = 6 (blocks in the row) + 2; %s"
          % ("the numpy restatement of the kernels' arithmetic, no device" if model_only else "device"))
    worst = {}
    over = 0

    def show(name, state, g):
        nonlocal over
        print(rc.line(name, state, g) + ("" if g["ratio"] <= 1.0 else "  OVER"), flush=True)
        k = kernel_of(name)
        worst[k] = max(worst.get(k, (0.0, "")), (g["ratio"], "%s %s" % (name, state)))
        over += not g["ratio"] <= 1.0

    for name in rc.SYMMETRIC_CASES + rc.FULL_CASES:
        got, _ = rc.run_case(pkg, name, model_only)
        for state, g in got.items():
            show(name, state, g)
    show("roof32", "iterate", roof_iterate(model_only))
    if model_only:
        for name in rc.WALK_CASES:
            got, _ = rc.run_case(pkg, name, True)
            for state, g in got.items():
                show(name, state, g)
    else:
        # FEMSHELL_SLICE_GRID is read once per process: the walking cases in a child of their own
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "walk.npz")
            subprocess.run([sys.executable, "-m", "tests.helpers.residual_cases", out] + list(rc.WALK_CASES), cwd=ROOT,
                           env=dict(os.environ, FEMSHELL_SLICE_GRID="8"), check=True, stdout=subprocess.DEVNULL, timeout=600)
            got = dict(np.load(out))
        for name in rc.WALK_CASES:
            for state in rt.STATES:
                show(name + " grid 8", state, {k: float(got["%s:%s:%s" % (k, name, state)]) for k in ("ratio", "ext", "cancel")})
    for k in sorted(worst):
        print("%-18s worst error / budget %.4f (%s)" % (k, worst[k][0], worst[k][1]))
    print("%d over the budget" % over)
    return 1 if over else 0


if __name__ == "__main__":
    sys.exit(main())
