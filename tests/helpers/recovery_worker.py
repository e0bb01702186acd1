"""The nodal recovery in a process of its own (tests/test_gpu_recovery.py): FEMSHELL_SLICE_GRID is read once per process.
    python tests/helpers/recovery_worker.py OUT.npz
The mesh: prescribed.panel(nx=20, ny=15, lift=True), 336 nodes in 11 slices (with a grid of 8 workgroups three of them take a second
slice), seeded u.  The npz holds nodes, elems, whether a second call gave the same bits, and the slice count of the plan."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.helpers import prescribed as pr, resultants as rs  # noqa: E402


def problem():
    xyz, tri = pr.panel(nx=20, ny=15, lift=True)
    return xyz, tri, rs.random_u(len(xyz), seed=47)


def main():
    out_file = sys.argv[1]
    pkg = importlib.import_module("fem-shell_amd")
    xyz, tri, u = problem()
    fs = pkg.FemShell(rs.NU, rs.E, rs.T, device=0)
    fs.set_mesh(xyz, tri)
    nodes, elems = fs.nodal_resultants(u)
    again = fs.nodal_resultants(u)
    same = np.array_equal(nodes, again[0]) and np.array_equal(elems, again[1])
    slices = pkg.build_plan(xyz, tri, None)["n_slices"]
    np.savez(out_file, nodes=nodes, elems=elems, same=int(same), slices=slices)
    fs.close()


if __name__ == "__main__":
    main()
