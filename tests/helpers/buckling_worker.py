"""The geometric product in a process of its own (tests/test_gpu_geometric_product.py): FEMSHELL_SLICE_GRID is read once per
process.
    python tests/helpers/buckling_worker.py OUT.npz
The mesh: prescribed.panel(nx=40, ny=30, lift=True), 1271 nodes in 40 slices, seeded u and a block X of five columns (a full pass
and a tail of one).  The npz holds Y, whether a second call gave the same bits, and the slice count of the plan."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.helpers import prescribed as pr, resultants as rs  # noqa: E402

COLS = 5


def problem():
    xyz, tri = pr.panel(nx=40, ny=30, lift=True)
    u = rs.random_u(len(xyz), seed=41)
    X = np.random.default_rng(43).uniform(-1.0, 1.0, (COLS, len(xyz), 6))
    return xyz, tri, u, X


def main():
    out_file = sys.argv[1]
    pkg = importlib.import_module("fem-shell_amd")
    xyz, tri, u, X = problem()
    fs = pkg.FemShell(rs.NU, rs.E, rs.T, device=0)
    fs.set_mesh(xyz, tri)
    Y = fs.geometric_product(u, X)
    same = np.array_equal(Y, fs.geometric_product(u, X))
    slices = pkg.build_plan(xyz, tri, None)["n_slices"]
    np.savez(out_file, Y=Y, same=int(same), slices=slices)
    fs.close()


if __name__ == "__main__":
    main()
