"""One rank of a row-partitioned context with shell sections on a shared GPU (tests/test_gpu_sections.py starts several of
these with FEMSHELL_RCCL_LIB pointing at the fake RCCL).  argv: rank world uid_file out_file"""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.helpers import sections  # noqa: E402


def main():
    rank, world = int(sys.argv[1]), int(sys.argv[2])
    uid_file, out_file = sys.argv[3], sys.argv[4]
    pkg = importlib.import_module("fem-shell_amd")
    cs = sections.three_strips(24, 40)
    fs = pkg.FemShell(0.3, 1e5, 0.05, device=0, rank=rank, world_size=world)
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
    cs.apply(fs)  # every rank passes the full arrays
    u, info = fs.solve(rtol=1e-13, max_it=100000)
    b, e = fs.row_range()
    rp, ci, vals, F = fs.export_bsr()
    np.savez(out_file, u=u, iterations=info["iterations"], converged=info["converged"], begin=b, end=e,
             k_cols=ci, k_vals=vals, k_F=F[:6 * (e - b)], assembly_kernel=fs.assembly_kernel())
    fs.close()


if __name__ == "__main__":
    main()
