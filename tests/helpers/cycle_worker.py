"""One multigrid cycle (femshell_pc_apply) in a process of its own, for the kernel choices a process reads once
(FEMSHELL_SPMV_NODE_WIDTH, FEMSHELL_SPMV_CHUNK): tests/test_gpu_cycle.py starts it with the knob in the
environment.  python -m tests.helpers.cycle_worker OUT.npz -- writes the cycle of the 48 x 48 panel (FP64 levels, K cycle) on the
random and the load vector, and its errors against the reference built from this process's own exports."""
import sys

import numpy as np

from tests.helpers import cycle_ref, meshes
from tests.helpers.product import ensure_built, pkg


def panel_context(n=48, coarsest_nodes=60, cycle="K"):
    ensure_built()
    m = meshes.structured(n, n, 0, 0, 10, 10, kind="t", ul_lr=True, bcids=(0, 0, 0, 0), factor=300.0, loading=2)
    fs = pkg.FemShell(0.3, 1e7, 0.5, device=0)
    fs.set_mesh(m.xyz, m.tri, m.quad)
    fs.set_dirichlet(m.dirichlet_mask())
    fs.set_loads(m.loads)
    fs.set_preconditioner("amg", cycle=cycle, coarsest_nodes=coarsest_nodes)
    return fs, m


def main(out):
    fs, m = panel_context()
    rng = np.random.default_rng(7)
    fs.assemble()
    r = rng.standard_normal(6 * m.n_nodes) * cycle_ref.free_dofs(fs)
    z = fs.pc_apply(r)
    F = fs.export_bsr()[3]
    zF = fs.pc_apply(F)
    levels, perm = cycle_ref.levels_from_context(fs)
    err = [cycle_ref.errors(z, cycle_ref.apply(levels, r, True, perm)), cycle_ref.errors(zF, cycle_ref.apply(levels, F, True, perm))]
    np.savez(out, z=z, zF=zF, err=np.array(err), levels=len(levels))
    fs.close()


if __name__ == "__main__":
    main(sys.argv[1])
