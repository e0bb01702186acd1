"""Elastic supports in a process of its own (tests/test_gpu_elastic_support.py): FEMSHELL_SLICE_GRID is read once per process, and
the ranks of a row partition are processes.
    python tests/helpers/elastic_support_worker.py RANK WORLD UID_FILE OUT.npz
The mesh: prescribed.panel(nx=40, ny=30, lift=True), 1271 nodes in 40 slices, a seeded foundation and springs, the edge x = 0
clamped, seeded nodal loads.  The npz holds S (the gathered support_stiffness), u (the block-Jacobi solution), the rank's rows of
K's diagonal blocks (from export_bsr), the rank's row range and the slice count of its plan.  WORLD > 1: launched with
FEMSHELL_RCCL_LIB pointing at the fake RCCL, like tests/helpers/element_loads_worker.py."""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.helpers import elastic_support as es, prescribed as pr  # noqa: E402

NU, E, T = 0.3, 2.1e5, 0.37


def problem():
    xyz, tri = pr.panel(nx=40, ny=30, lift=True)
    tk, _ = es.random_moduli(len(tri), 0, seed=17)
    springs = es.random_springs(len(xyz), seed=18)
    mask = np.zeros(len(xyz), np.uint8)
    mask[pr.edge_nodes(xyz, 0, 0.0)] = 0x3F
    nodal = np.random.default_rng(19).uniform(-1.0, 1.0, (len(xyz), 6))
    return xyz, tri, tk, springs, mask, nodal


def main():
    rank, world, uid_file, out_file = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    pkg = importlib.import_module("fem-shell_amd")
    xyz, tri, tk, springs, mask, nodal = problem()
    fs = pkg.FemShell(NU, E, T, device=0, rank=rank, world_size=world)
    if world > 1:
        if rank == 0:
            uid = pkg.comm_unique_id()
            np.save(uid_file + ".tmp.npy", uid)
            os.replace(uid_file + ".tmp.npy", uid_file)
        else:
            t0 = time.time()
            while not os.path.exists(uid_file):
                if time.time() - t0 > 60:
                    raise SystemExit("timeout waiting for the unique id")
                time.sleep(0.01)
            uid = np.load(uid_file)
        fs.comm_init(uid)
    fs.set_mesh(xyz, tri)
    fs.set_dirichlet(mask)
    fs.set_loads(nodal)
    fs.set_foundation(tk)
    fs.set_springs(*es.nodes_of(springs))
    S = fs.support_stiffness()
    same = np.array_equal(S, fs.support_stiffness())
    b, e = fs.row_range()
    u, info = fs.solve(rtol=1e-13, max_it=100000)
    rp, ci, vals, _ = fs.export_bsr()
    rp = rp[:e - b + 1]
    rows = np.repeat(np.arange(b, e), np.diff(rp))
    diag = vals[:len(rows)][ci[:len(rows)] == rows]
    slices = pkg.build_plan(xyz, tri, None, rank=rank, world_size=world)["n_slices"]
    np.savez(out_file, S=S, u=u, converged=info["converged"], diag=diag, begin=b, end=e, slices=slices, same=int(same))
    fs.close()


if __name__ == "__main__":
    main()
