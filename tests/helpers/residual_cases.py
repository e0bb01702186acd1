"""The cases of tests/test_gpu_residual_truth.py and tools/residual_truth_report.py: femshell_residual on the smallest shapes at which
each path of k_residual_dd_sym and k_residual_dd exists, every row against tests/helpers/residual_truth.py.

    python -m tests.helpers.residual_cases OUT.npz CASE [CASE ...]

runs cases in a process of its own (FEMSHELL_SLICE_GRID is read once per process) and writes, per case and state, the worst
error / budget over the rows ("ratio:<case>:<state>"), the same for amg_oracle.residual_extended ("ext:..."), how far the state
cancels ("cancel:..."), the residual itself ("r:...") and the slice count ("S:<case>").

Symmetric storage (k_residual_dd_sym):
  curved          sections.curved_patch(24, 18), 475 nodes: own rows, in-lists, the upper-triangle diagonal blocks
  curved-diag18   the same with FEMSHELL_DIAG_UPPER=0: the diagonal block read as any other
  curved-morton   the same under FEMSHELL_REORDER=morton: x and r pass through the permutation, rows meet other slots
  delaunay        meshes.delaunay_patch(3000, 2), partial masks: irregular widths, padded slots and in-list holes in every slice
  mixed           sections.mixed_patch(): quadrilaterals and triangles, three sections
  coil300-free, coil300-clamped   a hub row of 302 blocks, m = 1814, and its in-list of 301 entries (hub masks 0 and 0x3F)
  clique32        every node of a slice a neighbour of every other
  strip33         33 nodes: the last slice holds one node and 31 padded rows
Full storage (FEMSHELL_SYMMETRIC=0, k_residual_dd: x staged through LDS, chunks of four blocks with a tail):
  full-curved, full-strip33, full-coil40 / 41 / 62: rows of 42, 43 and 64 blocks -- under 64 KiB of x in LDS, over it, the widest
Slice walk (a child process under FEMSHELL_SLICE_GRID=8):
  walk-sym, walk-full   the 48 x 48 panel of tests/helpers/grid_worker.py, 76 slices: ten trips through the loop body"""
import os
import sys

import numpy as np

from oracle import amg_oracle
from tests.helpers import dynamics, meshes, sections
from tests.helpers import residual_truth as rt
from tests.helpers.product import ensure_built

NU, E, T = 0.3, 2.1e5, 0.04  # tests/test_gpu_limits.py, tests/test_gpu_modal.py
NO_QUADS = np.zeros((0, 4), np.int32)

SYMMETRIC_CASES = ("curved", "curved-diag18", "curved-morton", "delaunay", "mixed", "coil300-free", "coil300-clamped", "clique32",
                   "strip33")
FULL_CASES = ("full-curved", "full-coil40", "full-coil41", "full-coil62", "full-strip33")
WALK_CASES = ("walk-sym", "walk-full")
ENV = ("FEMSHELL_SYMMETRIC", "FEMSHELL_DIAG_UPPER", "FEMSHELL_REORDER", "FEMSHELL_ASM_PIPE", "FEMSHELL_SPMV_LOCAL")


def strip33():
    m = meshes.structured(10, 2, 0, 0, 5, 1, kind="t", ul_lr=True, bcids=(-1, -1, 1, -1))
    m.xyz[:, 2] = 0.2 * np.sin(0.8 * m.xyz[:, 0]) * np.cos(0.9 * m.xyz[:, 1])
    m.loads = np.random.default_rng(4).normal(size=(m.n_nodes, 6))
    return m


def problem(name):
    """(environment, xyz, tri, quad, dmask, loads, sections case or None, material)"""
    env = {"FEMSHELL_SYMMETRIC": "0"} if name.startswith("full-") or name == "walk-full" else {}
    base = name[5:] if name.startswith("full-") else name
    sec, mat = None, (NU, E, T)
    if base.startswith("curved"):
        m = sections.curved_patch(24, 18)
        if base == "curved-diag18":
            env["FEMSHELL_DIAG_UPPER"] = "0"
        if base == "curved-morton":
            env["FEMSHELL_REORDER"] = "morton"
        xyz, tri, quad, dmask, loads = m.xyz, m.tri, m.quad, m.dirichlet_mask(), m.loads
    elif base == "strip33":
        m = strip33()
        xyz, tri, quad, dmask, loads = m.xyz, m.tri, m.quad, m.dirichlet_mask(), m.loads
    elif base == "delaunay":  # the masks of tests/test_gpu_modal.py product_meshes
        xyz, tri = meshes.delaunay_patch(3000, 2)
        quad = NO_QUADS
        dmask = np.zeros(len(xyz), np.uint8)
        dmask[xyz[:, 0] < 0.2] = 0x3F
        dmask[::97] |= 0x07
        loads = np.random.default_rng(8).normal(size=(len(xyz), 6))
    elif base == "mixed":
        sec = sections.mixed_patch()
        xyz, tri, quad, dmask, loads = sec.xyz, sec.tri, sec.quad, sec.dmask, sec.loads
    elif base.startswith("walk"):
        from tests.helpers import grid_worker

        m = grid_worker.panel(48, 48)
        mat = grid_worker.MAT
        xyz, tri, quad, dmask = m.xyz, m.tri, m.quad, m.dirichlet_mask()
        loads = np.random.default_rng(6).normal(size=(m.n_nodes, 6))
    else:  # the meshes, masks and loads of tests/test_gpu_limits.py
        from tests.test_gpu_limits import constraints_and_loads, mesh_of

        mesh, _, hub_state = base.partition("-")
        xyz, tri, quad, hub = mesh_of(mesh)
        dmask, loads = constraints_and_loads(len(xyz), hub, 0x3F if hub_state == "clamped" else 0)
    return env, xyz, tri, quad, dmask, loads, sec, mat


class environment:
    """the switches a context reads when it is made, for the length of a block; the others of ENV unset"""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.before = {k: os.environ.get(k) for k in ENV}
        for k in ENV:
            os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.before.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def expectations(name, plan, rowptr):
    """the path the case is there for"""
    full = name.startswith("full-") or name == "walk-full"
    assert plan["symmetric"] == (0 if full else 1), (name, plan["symmetric"])
    widest = int(np.diff(rowptr).max())
    if "coil" in name:
        assert widest == int(name.split("coil")[1].split("-")[0]) + 2
    if name.startswith("full-"):
        lds = plan["max_slice_width"] * 32 * 48
        assert plan["max_slice_width"] == widest and (lds > 65536) == (name in ("full-coil41", "full-coil62")), (name, lds)
    if "strip33" in name:
        assert len(rowptr) - 1 == 33 and plan["n_slices"] == 2
    if name.startswith("walk"):
        assert plan["n_slices"] == 76


def run_case(pkg, name, model_only=False):
    """{state: dict(ratio, ext, cancel, r, truth, budget)} and the slice count.  model_only: no device -- K and F from the oracle's
    assembly, the residual from rt.model in the kernel's order of the terms."""
    env, xyz, tri, quad, dmask, loads, sec, mat = problem(name)
    n = len(xyz)
    free = dynamics.free_dofs(dmask, n)
    with environment(env):
        plan = pkg.build_plan(xyz, tri, quad)
        if model_only:
            from tests.helpers import oracle

            r, c, v, F0 = (sections.reference(sec) if sec is not None
                           else oracle.assemble(xyz, tri, quad, oracle.material(*mat), dmask, loads))
            fs = None
        else:
            fs = pkg.FemShell(*mat, device=0)
            if sec is not None:
                sec.apply(fs)
            else:
                fs.set_mesh(xyz, tri, quad)
                fs.set_dirichlet(dmask)
                fs.set_loads(loads)
            fs.assemble()
            r, c, v, F0 = fs.export_bsr()
    expectations(name, plan, r)
    K = (r, c, v)
    M = rt.csr(K)
    order = "sym" if plan["symmetric"] else "stored"
    got = {}
    for state, (x, F_want) in rt.states(K, F0, free).items():
        if fs is None:
            F, res = F_want, rt.model(K, F_want, x, order=order)
        else:
            fs.set_loads(F_want.reshape(n, 6))
            res = fs.residual(x)
            F = fs.export_bsr()[3]
            np.testing.assert_array_equal(F, F_want)  # nodal loads reach F as they are (zero on the constrained dofs)
            np.testing.assert_array_equal(fs.export_bsr()[2], v)
        truth = rt.exact(K, F, x)
        budget = rt.bound(K, F, x, truth)
        ext = amg_oracle.residual_extended(M, F, x)
        got[state] = dict(ratio=float(rt.ratios(res, truth, budget).max()), ext=float(rt.ratios(ext, truth, budget).max()),
                          cancel=rt.cancellation(truth, rt.scale(K, F, x)), r=res, truth=truth, budget=budget)
    if fs is not None:
        fs.close()
    return got, int(plan["n_slices"])


def line(name, state, g):
    return ("%-16s %-7s ||r*|| / ||S|| %.1e   worst error / budget %s   residual_extended / budget %.3g"
            % (name, state, g["cancel"], ("%.4f" if g["ratio"] < 10.0 else "%.3g") % g["ratio"], g["ext"]))


def main(path, names):
    pkg = ensure_built()
    out = {}
    for name in names:
        got, slices = run_case(pkg, name)
        out["S:" + name] = slices
        for state, g in got.items():
            print(line(name, state, g), flush=True)
            for key in ("ratio", "ext", "cancel", "r"):
                out["%s:%s:%s" % (key, name, state)] = g[key]
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
