"""Thermal loads in a process of its own (tests/test_gpu_thermal.py): FEMSHELL_SLICE_GRID is read once per process, and the ranks
of a row partition are processes.
    python tests/helpers/thermal_worker.py RANK WORLD UID_FILE OUT.npz
The mesh: prescribed.panel(nx=40, ny=30, lift=True), 1271 nodes in 40 slices, seeded temperatures, element loads and nodal loads.
The npz holds T (the gathered thermal_load_vector), S (the gathered element_load_vector), F (the rank's rows of the right-hand side
under a Dirichlet set, from export_bsr), the rank's row range and the slice count of its plan.  WORLD > 1: launched with
FEMSHELL_RCCL_LIB pointing at the fake RCCL, like tests/helpers/element_loads_worker.py."""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.helpers import element_loads as el, prescribed as pr, thermal as th  # noqa: E402

NU, E, T = 0.3, 2.1e5, 0.37
ALPHA = 1.2e-5


def problem():
    xyz, tri = pr.panel(nx=40, ny=30, lift=True)
    tt, _ = th.random_temps(len(tri), 0, seed=29)
    tl, _ = el.random_loads(len(tri), 0, seed=17)
    mask = np.zeros(len(xyz), np.uint8)
    mask[pr.edge_nodes(xyz, 0, 0.0)] = 0x3F
    nodal = np.random.default_rng(19).uniform(-1.0, 1.0, (len(xyz), 6))
    return xyz, tri, tt, tl, mask, nodal


def main():
    rank, world, uid_file, out_file = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    pkg = importlib.import_module("fem-shell_amd")
    xyz, tri, tt, tl, mask, nodal = problem()
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
    fs.set_element_loads(tl)
    fs.set_expansion(ALPHA)
    fs.set_thermal(tt)
    Tv = fs.thermal_load_vector()
    same = np.array_equal(Tv, fs.thermal_load_vector())
    S = fs.element_load_vector()
    b, e = fs.row_range()
    fs.assemble()
    F = fs.export_bsr()[3][:6 * (e - b)]
    slices = pkg.build_plan(xyz, tri, None, rank=rank, world_size=world)["n_slices"]
    np.savez(out_file, T=Tv, S=S, F=F, begin=b, end=e, slices=slices, same=int(same))
    fs.close()


if __name__ == "__main__":
    main()
