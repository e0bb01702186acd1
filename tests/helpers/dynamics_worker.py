"""One rank of a row-partitioned Newmark run on a shared GPU (tests/test_gpu_dynamics.py launches several of these with
FEMSHELL_RCCL_LIB pointing at the fake RCCL, beside tests/helpers/multirank_worker.py).  The run: sections.three_strips() with
section densities, the default scheme from the static deflection with the load removed, N accepted steps.
argv: rank world uid_file out_file dt steps"""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.helpers import oracle, sections  # noqa: E402

NU, E, T = 0.3, 2.1e5, 0.04
SECTION_RHO = np.array([7.8e-3, 2.7e-3, 4.4e-3])


def main():
    rank, world = int(sys.argv[1]), int(sys.argv[2])
    uid_file, out_file, dt, steps = sys.argv[3], sys.argv[4], float(sys.argv[5]), int(sys.argv[6])
    pkg = importlib.import_module("fem-shell_amd")
    cs = sections.three_strips()
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
    cs.apply(fs)
    fs.set_preconditioner("jacobi")
    fs.set_density(0.0, section_rho=SECTION_RHO)
    mass = fs.lumped_mass()
    # the static deflection from the reference of the sectioned K (every rank computes the same one)
    r, c, v, F = sections.reference(cs)
    u0 = oracle.direct_solve(r, c, v, F).reshape(-1, 6)
    fs.set_loads(np.zeros_like(cs.loads))
    fs.dynamics_begin(dt, u0=u0)
    us, energies = [fs.dynamics_state()[0]], [fs.dynamics_energy()]
    for _ in range(steps):
        info = fs.dynamics_step(rtol=1e-12, max_it=20000)
        assert info["converged"] == 1, info
        fs.dynamics_accept()
        us.append(fs.dynamics_state()[0])
        energies.append(fs.dynamics_energy())
    u, vel, acc = fs.dynamics_state()
    b, e = fs.row_range()
    np.savez(out_file, us=np.array(us), u=u, v=vel, a=acc, energies=np.array(energies), mass=mass, begin=b, end=e)
    fs.dynamics_end()
    fs.close()


if __name__ == "__main__":
    main()
