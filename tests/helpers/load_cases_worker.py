"""Load cases in a process of its own (tests/test_gpu_load_cases.py): FEMSHELL_SLICE_GRID is read once per process.
    python tests/helpers/load_cases_worker.py OUT.npz
On delaunay600_rcm (19 slices) and coil300 (10 slices) of tests/helpers/resultants.py: the seven cases of load_cases.case_loads in
one call and each in a call of its own, block-Jacobi, to rtol 1e-12 and after exactly 1, 2 and 5 iterations.  Asserts here that
every case is bit for bit what it is alone and that two calls agree; the npz holds, per mesh, u and the iteration counts of the
converged call, the grid of the per-slice kernels and the slices a workgroup walks."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.helpers import load_cases as lc, resultants as rs  # noqa: E402

N_ALL = 7


def main():
    out_file = sys.argv[1]
    pkg = importlib.import_module("fem-shell_amd")
    cap = pkg.grid_cap(os.environ.get("FEMSHELL_SLICE_GRID"), 65536)
    out = {}
    for name in ("delaunay600_rcm", "coil300"):
        xyz, tri, quad, sec, env = rs.device_meshes()[name]()
        os.environ.update(env)
        fs = pkg.FemShell(rs.NU, rs.E, rs.T)
        fs.set_mesh(xyz, tri, quad)
        mask = lc.mask_for(name, len(xyz))
        fs.set_dirichlet(mask)
        L = lc.case_loads(len(xyz), mask, N_ALL)
        for rtol, max_it in ((1e-12, 20000), (0.0, 1), (0.0, 2), (0.0, 5)):
            u, cases, info = fs.solve_cases(L, rtol=rtol, max_it=max_it)
            assert info["passes"] == 2 and info["fused_product"] == 1, info
            for j in range(N_ALL):
                ua, ca, _ = fs.solve_cases(L[j], rtol=rtol, max_it=max_it)
                assert np.array_equal(ua[0], u[j]) and ca[0] == cases[j], (name, rtol, max_it, j, ca[0], cases[j])
            u2, cases2, _ = fs.solve_cases(L[::-1], rtol=rtol, max_it=max_it)
            assert np.array_equal(u2[::-1], u) and cases2[::-1] == cases, (name, rtol, max_it)
            if rtol > 0.0:
                assert all(c["converged"] == 1 for c in cases), cases
                assert cases[0]["iterations"] != cases[1]["iterations"] and cases[2]["iterations"] == 0
                out["u_" + name] = u
                out["it_" + name] = np.array([c["iterations"] for c in cases])
        slices = pkg.build_plan(xyz, tri, quad)["n_slices"]
        grid = min(8 * ((slices + 7) // 8), cap)
        out["grid_" + name] = grid
        out["walks_" + name] = -(-((slices + 7) // 8) // (grid // 8))
        fs.close()
    np.savez(out_file, **out)


if __name__ == "__main__":
    main()
