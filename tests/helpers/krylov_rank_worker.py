"""One rank of the two-rank Krylov probes (tests/test_gpu_krylov_truth.py, with tests/helpers/fake_rccl as the other multi-rank
tests): the start and one probe-chained iteration of the single-reduction recurrence and the two dots of the flexible one on a
row-partitioned context; what comes back -- the all-reduced red[], the lengths the product reports, the rank's owned rows of
the vectors -- goes to the test, which holds the sums to exact dots over the owned rows of all ranks.
argv: rank world uid_file out_file symmetric"""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.helpers import krylov_cases as kc  # noqa: E402
from tests.helpers import krylov_truth as kt  # noqa: E402

MESH = "curved"


def main():
    rank, world = int(sys.argv[1]), int(sys.argv[2])
    uid_file, out_file = sys.argv[3], sys.argv[4]
    symmetric = os.environ.get("FEMSHELL_SYMMETRIC", "1") != "0"
    pkg = importlib.import_module("fem-shell_amd")
    xyz, tri, quad, dmask, loads, mat = kc.mesh(MESH)
    fs = pkg.FemShell(*mat, device=0, rank=rank, world_size=world)
    if rank == 0:
        np.save(uid_file + ".tmp.npy", pkg.comm_unique_id())
        os.replace(uid_file + ".tmp.npy", uid_file)
    t0 = time.time()
    while not os.path.exists(uid_file):
        if time.time() - t0 > 60:
            raise SystemExit("timeout waiting for the unique id")
        time.sleep(0.01)
    fs.comm_init(np.load(uid_file))
    fs.set_mesh(xyz, tri, quad)
    fs.set_dirichlet(dmask)
    fs.set_loads(loads)
    fs.solve(rtol=0.0, max_it=1)  # (assembles and builds the block-Jacobi inverse: the probes build nothing)
    G = fs.krylov_grid()
    P = kt.PHASES
    gather = 1 if symmetric else 0
    out = {"own": fs.owned_nodes(), "G": G}

    def keep(tag, *names):
        s = fs.krylov_get("scalars")
        out[tag + "_red"] = np.array(s.red[:])
        out[tag + "_done"] = s.done
        for v in names:
            out["%s_%s" % (tag, v)] = fs.krylov_get(v)

    kc.set_scalars(fs, kt.Scalars())
    fs.krylov_launch("cgcg_init")
    out["len3_init"] = fs.krylov_launch("product", 1, gather)[0]
    if gather:  # (the sums are the product's; the whole q is for the test's eyes: the update kernel collects it by itself)
        out["init_q_direct"] = fs.krylov_get("q")
    fs.krylov_launch("scalar_step", 3, P["fused_init"], G, out["len3_init"] or G, -1)
    keep("init", "r", "z")
    fs.krylov_launch("cgcg_update", -1, gather)
    out["len3_step"] = fs.krylov_launch("product", 1, gather)[0]
    fs.krylov_launch("scalar_step", 3, P["fused_step"], G, out["len3_step"] or G, -1)
    keep("step", "r", "z", "x", "p", "sv")
    # the whole w = K z of the last product, by a product that gathers (its sums go to the same place and are not looked at)
    fs.krylov_launch("product", 1, 0)
    out["step_q"] = fs.krylov_get("q")
    # the two dots of the flexible recurrence's error estimate
    out["two_dots"] = fs.krylov_launch("two_dots", 0, 1)[2]
    np.savez(out_file, **out)
    fs.close()


if __name__ == "__main__":
    main()
