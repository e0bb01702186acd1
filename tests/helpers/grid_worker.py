"""The library's per-slice kernels under one grid setting, in a process of its own: FEMSHELL_SLICE_GRID and FEMSHELL_ASM_GRID are
read once per process, so tests/test_gpu_slice_walk.py starts this worker once per setting.
    python -m tests.helpers.grid_worker OUT.npz [SECTIONS]
SECTIONS: letters of the sections to run (default "abcde"):
  a  panels of 1, 7, 8, 9, 15, 17 and 76 slices, symmetric and full storage: spmv, spmm, residual, element_product, reactions, K, F
  b  the two-phase assembly kernel (FEMSHELL_ASM_PIPE=0) on the 76-slice panel and a mixed mesh
  c  block-Jacobi CG, classic and single-reduction, on the 76-slice panel
  d  one multigrid cycle in every storage and precision of the levels, and a multigrid solve
  e  modal_gram, modes, Newmark steps
What the npz holds, by prefix of the key:
  S:<matrix>     slice count of every matrix touched (level operators: ceil(n_nodes / 32))
  bits:<case>    a result formed row by row by one lane whichever workgroup holds the slice: the same bits under every grid
  close:<case>   a result that passes through partial sums over workgroups (CG and multigrid solutions, Gram matrices): compared
                 with the default grid's by the test
  its:<case>     an iteration count
  ratio:<case>   an error against a reference over its bound, measured here: at most 1
  same:<case>    1 where two runs in this process gave the same bits
  text:<case>    a string
The bounds are the project's: products |err_i| <= 2 n_i eps (|K||x|)_i (tests/test_gpu_modal.py, tests/test_gpu_limits.py),
residual 1e-11 ||F|| against amg_oracle.residual_extended, K 1e-12 per stored block against the oracle, F exact, the element
product and the reactions 1e-12 S_a per node row (tests/test_gpu_prescribed.py), CG and cycles as named at each section."""
import os
import sys
import time

import numpy as np

from oracle import amg_oracle
from tests.helpers import cycle_ref, dynamics, meshes, modal, oracle, prescribed, sections
from tests.helpers.product import ensure_built, pkg

EPS = np.finfo(np.float64).eps
MAT = (0.3, 1e7, 0.5)
# (nx, ny) of the structured triangle panels and the slices of their plans: below, at and just above one and two rows of eight
# workgroups; 2401 nodes: the last slice holds one node
PANELS = [((4, 4), 1), ((12, 15), 7), ((15, 15), 8), ((12, 21), 9), ((20, 21), 15), ((22, 22), 17), ((48, 48), 76)]

out = {}


class environment:
    """os.environ with the given variables for the length of a block (the library reads these per context or per call)"""

    def __init__(self, **env):
        self.env = env

    def __enter__(self):
        self.before = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def ratio(name, value, bound):
    r = float(value) / float(bound)
    out["ratio:" + name] = r
    print("[grid] %-52s %.3e of its bound %.1e" % (name, r, bound), flush=True)


def panel(nx, ny):
    m = meshes.structured(nx, ny, 0, 0, 10, 10, kind="t", ul_lr=True, bcids=(0, 0, 0, 0), factor=300.0, loading=2)
    m.xyz[:, 2] = 0.3 * np.sin(0.9 * m.xyz[:, 0]) * np.cos(0.7 * m.xyz[:, 1])  # (membrane and bending rows couple)
    return m


def mixed_mesh():
    """40 x 40 squares, half of them cut into triangles (tests/test_gpu_cycle.py "mixed")"""
    m = meshes.structured(40, 40, 0, 0, 10, 10, kind="q", bcids=(1, 1, 1, 1), factor=300.0, loading=2)
    half = len(m.quad) // 2
    tri = np.concatenate([m.quad[half:, [0, 1, 2]], m.quad[half:, [0, 2, 3]]]).astype(np.int32)
    return m.xyz, tri, m.quad[:half], m.dirichlet_mask(), m.loads


def context(xyz, tri, quad, dmask, loads, mat=MAT, flags=None):
    fs = pkg.FemShell(*mat, device=0) if flags is None else pkg.FemShell(*mat, flags=flags, device=0)
    fs.set_mesh(xyz, tri, quad)
    fs.set_dirichlet(dmask)
    fs.set_loads(loads)
    return fs


def worst_block(v, v0):
    """max over the stored blocks of max|K_b - K_b^ref| / max|K_b^ref| (tests/test_gpu_limits.py); a zero block must be zero"""
    d, s = np.abs(v - v0).max(axis=(1, 2)), np.abs(v0).max(axis=(1, 2))
    return float("inf") if np.any(d[s == 0.0] != 0.0) else float((d[s > 0.0] / s[s > 0.0]).max())


def assembled_against_the_oracle(name, fs, ref):
    r0, c0, v0, F0 = ref
    r, c, v, F = fs.export_bsr()
    out["bits:%s:K" % name], out["bits:%s:F" % name] = v, F
    out["same:%s:pattern" % name] = int(np.array_equal(r, r0) and np.array_equal(c, c0))
    out["same:%s:F_is_the_oracles" % name] = int(np.array_equal(F, F0))
    ratio(name + ":K", worst_block(v, v0), 1e-12)
    return r, c, v, F


# ------------------------------------------------------------------ a. products and assembly on panels of 1 to 76 slices

def section_a():
    for (nx, ny), slices in PANELS:
        m = panel(nx, ny)
        n = m.n_nodes
        dmask = m.dirichlet_mask()
        mat = oracle.material(*MAT)
        ref = oracle.assemble(m.xyz, m.tri, m.quad, mat, dmask, m.loads)
        K_unc = oracle.assemble(m.xyz, m.tri, m.quad, mat, None, None)[:3]
        free = dynamics.free_dofs(dmask, n)
        X = np.random.default_rng(5).normal(size=(5, 6 * n)) * free
        xu = np.random.default_rng(7).uniform(-1.0, 1.0, 6 * n)
        for sym in ("1", "0"):
            name = "a:S%d:sym%s" % (slices, sym)
            with environment(FEMSHELL_SYMMETRIC=sym):
                out["S:" + name] = pkg.build_plan(m.xyz, m.tri)["n_slices"]
                fs = context(m.xyz, m.tri, m.quad, dmask, m.loads)
            fs.assemble()
            r, c, v, F = assembled_against_the_oracle(name, fs, ref)
            K = dynamics.to_matrix((r, c, v))
            K.sort_indices()
            data, starts = K.data.astype(np.longdouble), K.indptr[:-1]
            want = np.stack([np.add.reduceat(data * x.astype(np.longdouble)[K.indices], starts) for x in X])
            bound = np.maximum(2.0 * np.repeat(6.0 * np.diff(r), 6) * EPS * (abs(K) @ np.abs(X).T).T, 1e-300)
            y = out["bits:%s:spmv" % name] = fs.spmv(X[0])
            ratio(name + ":spmv", (np.abs(y - want[0]) / bound[0]).max(), 1.0)
            worst = 0.0
            for nc in (1, 3, 4, 5):
                Y = out["bits:%s:spmm%d" % (name, nc)] = fs.spmm(X[:nc])
                worst = max(worst, float((np.abs(Y - want[:nc]) / bound[:nc]).astype(np.float64).max()))
            ratio(name + ":spmm", worst, 1.0)
            nb = np.linalg.norm(F)
            x = X[0] * (nb / np.linalg.norm(K @ X[0]))  # (K x of the size of F: tests/test_gpu_limits.py)
            res = out["bits:%s:residual" % name] = fs.residual(x)
            ratio(name + ":residual", np.linalg.norm(res - amg_oracle.residual_extended(K, F, x)), 1e-11 * nb)
            scale = 1e-12 * prescribed.row_scale(K_unc, xu)
            ye = out["bits:%s:element_product" % name] = fs.element_product(xu)
            ratio(name + ":element_product", (np.abs(ye - oracle.spmv(*K_unc, xu)).reshape(-1, 6).max(axis=1) / scale).max(), 1.0)
            re = out["bits:%s:reactions" % name] = fs.reactions(xu.reshape(n, 6))
            ratio(name + ":reactions", (np.abs(re - prescribed.reactions(K_unc, xu, m.loads)).max(axis=1) / scale).max(), 1.0)
            fs.close()


# ------------------------------------------------------------------ b. the two-phase assembly kernel

def section_b():
    m = panel(48, 48)
    cases = {"b:panel76": (m.xyz, m.tri, m.quad, m.dirichlet_mask(), m.loads), "b:mixed": mixed_mesh()}
    for name, (xyz, tri, quad, dmask, loads) in cases.items():
        with environment(FEMSHELL_ASM_PIPE="0"):
            out["S:" + name] = pkg.build_plan(xyz, tri, quad)["n_slices"]
            fs = context(xyz, tri, quad, dmask, loads)
        out["text:%s:kernel" % name] = fs.assembly_kernel()
        fs.assemble()
        assembled_against_the_oracle(name, fs, oracle.assemble(xyz, tri, quad, oracle.material(*MAT), dmask, loads))
        fs.close()


# ------------------------------------------------------------------ c. block-Jacobi CG

def section_c():
    """tests/test_gpu_parity.py test_cg_follows_oracle_cg_iteration_by_iteration on the 76-slice panel: the first 60 entries of
    the residual history at rtol 1e-6 against oracle.pcg, the iteration count within 3 of the oracle's.  The flat panel, as there.
    The solution the test compares with the default grid's comes from a solve to rtol 1e-12, whose solver term smoke() and
    tests/test_gpu_parity.py hold to 1e-10 against a direct solve."""
    m = meshes.structured(48, 48, 0, 0, 10, 10, kind="t", ul_lr=True, bcids=(0, 0, 0, 0), factor=300.0, loading=2)
    r0, c0, v0, F0 = oracle.assemble(m.xyz, m.tri, m.quad, oracle.material(*MAT), m.dirichlet_mask(), m.loads)
    _, info0 = oracle.pcg(r0, c0, v0, F0, rtol=1e-10, max_it=20000, history=True)
    fs = context(m.xyz, m.tri, m.quad, m.dirichlet_mask(), m.loads)
    fs.set_preconditioner("jacobi")
    out["S:c:panel76"] = pkg.build_plan(m.xyz, m.tri)["n_slices"]
    for name, single in (("c:classic", "0"), ("c:single_reduction", "1")):
        with environment(FEMSHELL_CG_SINGLE_REDUCTION=single):
            u, info = fs.solve(rtol=1e-10, max_it=20000)
            h = fs.residual_history()
            u2, info2 = fs.solve(rtol=1e-10, max_it=20000)
            h2 = fs.residual_history()
            ut, infot = fs.solve(rtol=1e-12, max_it=20000)
        out["close:%s:u" % name], out["its:" + name] = ut, info["iterations"]
        out["same:%s:converged_to_1e-12" % name] = int(infot["converged"] == 1)
        out["same:%s:converged" % name] = int(info["converged"] == 1 and info0["converged"] == 1)
        out["same:%s:two_solves" % name] = int(np.array_equal(u, u2) and np.array_equal(h, h2) and info["iterations"] == info2["iterations"])
        k = min(len(h), len(info0["history"]), 60)
        ratio(name + ":history", (np.abs(h[:k] - info0["history"][:k]) / np.abs(info0["history"][:k])).max(), 1e-6)
        ratio(name + ":iterations", abs(info["iterations"] - info0["iterations"]), 3)
    fs.close()


# ------------------------------------------------------------------ d. one multigrid cycle

def cycle_case(name, kind, n, env, cycle, mode, tol, coarsest_nodes=60, flags=None, want_solve=False):
    """pc_apply on a random vector and on the load vector against the restatement on the exported hierarchy (tests/test_gpu_cycle.py
    _check_against_reference and _properties): relative 2-norm and worst node within tol; with TOL_VEC at least 100 x TOL_F32 away
    from the values-only model; M(2r) = 2 M(r) and a repeated call bit for bit."""
    from tests.test_gpu_cycle import _mesh
    xyz, tri, quad, dmask, loads, mat = _mesh(kind, n)
    with environment(**env):
        fs = context(xyz, tri, quad, dmask, loads, mat, flags)
        fs.assemble()
        fs.set_preconditioner("amg", cycle=cycle, coarsest_nodes=coarsest_nodes)
        r = np.random.default_rng(11).standard_normal(6 * fs.n_nodes) * cycle_ref.free_dofs(fs)
        vecs = {"random": r, "load": fs.export_bsr()[3]}
        zs = {v: fs.pc_apply(x) for v, x in vecs.items()}
        levels, perm = cycle_ref.levels_from_context(fs, float_mode=mode)
        lv = fs.amg_levels()
        out["S:" + name] = np.array([(l["n_nodes"] + 31) // 32 for l in lv])
        out["its:%s:levels" % name] = len(lv)
        if name.startswith("d:delaunay"):  # (a restriction row of more than 64 fine nodes: wider than the LDS panel of k_spmv)
            out["its:%s:widest_restriction_row" % name] = int(np.diff(levels[-2].R.tocsr().indptr).max() // 6)
        for v, x in vecs.items():
            rel, node = cycle_ref.errors(zs[v], cycle_ref.apply(levels, x, cycle == "K", perm))
            ratio("%s:%s" % (name, v), max(rel, node), tol)
            if tol == cycle_ref.TOL_VEC:
                ratio("%s:%s:vectors_were_rounded" % (name, v), 100.0 * cycle_ref.TOL_F32, rel)
        z1 = fs.pc_apply(r)
        out["same:%s:repeated" % name] = int(np.array_equal(z1, zs["random"]))
        out["same:%s:doubled" % name] = int(np.array_equal(fs.pc_apply(2.0 * r), 2.0 * z1))
        if want_solve:
            u, info = fs.solve(rtol=1e-10, max_it=400)
            out["close:%s:u" % name], out["its:%s:solve" % name] = u, info["iterations"]
            out["same:%s:converged" % name] = int(info["converged"] == 1)
        fs.close()


def section_d():
    T64, T32, TV = cycle_ref.TOL_FP64, cycle_ref.TOL_F32, cycle_ref.TOL_VEC
    F64 = {"FEMSHELL_AMG_SMOOTH_F32": "0"}
    F32 = {"FEMSHELL_AMG_SMOOTH_F32": "3", "FEMSHELL_AMG_VEC_F32": "0"}
    for storage, sym in (("sym", "1"), ("full", "100000")):
        for cyc in "VK":
            cycle_case("d:fp64-%s-%s" % (storage, cyc), "panel", 48, dict(F64, FEMSHELL_AMG_COARSE_SYM=sym), cyc, 0, T64,
                       want_solve=(storage == "sym" and cyc == "K"))
        cycle_case("d:f32-vec0-%s-K" % storage, "panel", 48, dict(F32, FEMSHELL_AMG_COARSE_SYM=sym), "K", 3, T32)
    cycle_case("d:f32-vec2-sym-K", "panel", 48,
               {"FEMSHELL_AMG_SMOOTH_F32": "3", "FEMSHELL_AMG_VEC_F32": "2", "FEMSHELL_AMG_COARSE_SYM": "1"}, "K", 3, TV)
    for fuse in ("0", "-1"):  # (full-storage coarse levels: the Chebyshev start in k_spmv's epilogue, or a pass of its own)
        cycle_case("d:fuse%s-full-K" % fuse, "panel", 48, dict(F64, FEMSHELL_AMG_COARSE_SYM="100000", FEMSHELL_AMG_FUSE=fuse), "K", 0, T64)
    # tests/test_gpu_cycle.py test_morton_numbered_delaunay_shell_with_rows_wider_than_the_lds_panel, its 1e-10
    cycle_case("d:delaunay-morton-K", "delaunay", 2500, dict(F64, FEMSHELL_AMG_PATCH_TAU="0"), "K", 0, 1e-10, coarsest_nodes=200,
               flags=pkg.REF_DEFAULT | pkg.REORDER_MORTON)


# ------------------------------------------------------------------ e. modal analysis and dynamics

NU, E, T, RHO = 0.3, 2.1e5, 0.04, 7.8e-3  # tests/test_gpu_modal.py, tests/test_gpu_dynamics.py


def modes_case(name, nx, ny, pc, n_modes=4, tol=1e-6, max_it=3000):
    """tests/test_gpu_modal.py check_modes for n_modes pairs: eigenvalues within 1e-8, shapes within 1e-3 of the reference's
    cluster, mass-orthonormal to 1e-10, residuals within 2 tol"""
    m = sections.curved_patch(nx, ny)
    dmask = m.dirichlet_mask()
    mass = dynamics.lumped_mass(m.xyz, m.tri, m.quad, RHO, T)
    fs = context(m.xyz, m.tri, m.quad, dmask, m.loads, (NU, E, T))
    fs.set_density(RHO)
    fs.set_preconditioner("jacobi") if pc == "jacobi" else fs.set_preconditioner("amg", coarsest_nodes=100)
    out["S:" + name] = pkg.build_plan(m.xyz, m.tri, m.quad)["n_slices"]
    fs.assemble()
    K = dynamics.to_matrix(fs.export_bsr()[:3])
    lam_ref, X_ref = modal.reference(K, mass, dmask, n_modes + 4, 0.0)
    lam, shapes, res, info = fs.modes(n_modes, tol=tol, max_it=max_it)
    X = shapes.reshape(n_modes, -1)
    out["same:%s:converged" % name] = int(info["converged"] == n_modes and (np.diff(lam) >= 0.0).all()
                                          and (X[:, ~dynamics.free_dofs(dmask, m.n_nodes)] == 0.0).all())
    ratio(name + ":lambda", (np.abs(lam - lam_ref[:n_modes]) / lam_ref[:n_modes]).max(), 1e-8)
    groups = modal.clusters(lam_ref, 0.0)
    ratio(name + ":shapes", max(modal.subspace_distance(X[j], X_ref[modal.cluster_of(j, groups)], mass) for j in range(n_modes)), 1e-3)
    ratio(name + ":orthonormal", np.abs((X * np.asarray(mass).ravel()) @ X.T - np.eye(n_modes)).max(), 1e-10)
    ratio(name + ":residuals", max(modal.residual_norms(K, mass, dmask, lam, X, 0.0).max() / 2.0, res.max()), tol)
    a = fs.modes(n_modes, tol=tol, max_it=max_it)
    out["same:%s:two_runs" % name] = int(np.array_equal(a[0], lam) and np.array_equal(a[1], shapes))
    fs.close()


def section_e():
    # modal_gram on the 76-slice panel against its dot-product bound (tests/test_gpu_modal.py), twice the same bits
    m = panel(48, 48)
    fs = context(m.xyz, m.tri, m.quad, m.dirichlet_mask(), m.loads, (NU, E, T))
    fs.set_density(RHO)
    out["S:e:gram"] = pkg.build_plan(m.xyz, m.tri)["n_slices"]
    mass = dynamics.lumped_mass(m.xyz, m.tri, m.quad, RHO, T).ravel()
    n = 6 * m.n_nodes
    rng = np.random.default_rng(9)
    worst, same = 0.0, True
    for qa, qb in ((1, 1), (5, 3), (24, 24)):
        A, B = rng.normal(size=(qa, n)), rng.normal(size=(qb, n))
        for weighted in (True, False):
            w = mass if weighted else np.ones(n)
            G = fs.modal_gram(A, B, weighted)
            out["close:e:gram:%d-%d-%d" % (qa, qb, weighted)] = G
            worst = max(worst, (np.abs(G - (A * w) @ B.T) / (2.0 * n * EPS * ((np.abs(A) * w) @ np.abs(B).T))).max())
            same = same and np.array_equal(G, fs.modal_gram(A, B, weighted))
    ratio("e:gram", worst, 1.0)
    out["same:e:gram:repeated"] = int(same)
    fs.close()
    modes_case("e:modes-small-jacobi", 12, 10, "jacobi")
    modes_case("e:modes-curved-amg", 24, 18, "amg", max_it=360)
    # five Newmark steps of the "default" case of tests/test_gpu_dynamics.py on its large patch (multigrid): N tau, N = 5
    from tests.test_gpu_dynamics import first_period
    m = sections.curved_patch(44, 40)
    dmask = m.dirichlet_mask()
    fs = context(m.xyz, m.tri, m.quad, dmask, m.loads, (NU, E, T))
    fs.set_density(RHO)
    fs.set_preconditioner("amg")
    out["S:e:newmark"] = pkg.build_plan(m.xyz, m.tri, m.quad)["n_slices"]
    fs.assemble()
    bsr = fs.export_bsr()
    nn = m.n_nodes
    u0 = oracle.direct_solve(*bsr).reshape(nn, 6)
    dt = first_period()[0] / 20.0
    ref = dynamics.Newmark(dynamics.to_matrix(bsr), dynamics.lumped_mass(m.xyz, m.tri, m.quad, RHO, T), dmask, dt)
    zero = np.zeros((nn, 6))
    fs.set_loads(zero)
    fs.dynamics_begin(dt, u0=u0)
    want = [ref.begin(zero.ravel(), u0, None)]
    got = [fs.dynamics_state()[0].ravel()]
    steps = 5
    for _ in range(steps):
        info = fs.dynamics_step(rtol=1e-12, max_it=20000)
        assert info["converged"] == 1, info
        fs.dynamics_accept()
        got.append(fs.dynamics_state()[0].ravel())
        want.append(ref.step(zero.ravel()))
    out["its:e:newmark:levels"] = info["amg_levels"]
    ratio("e:newmark", max(np.abs(g - w[0]).max() for g, w in zip(got, want)), steps * 1e-9 * max(np.abs(w[0]).max() for w in want))
    fs.dynamics_end()
    fs.close()


def main(path, which):
    ensure_built()
    for letter, run in (("a", section_a), ("b", section_b), ("c", section_c), ("d", section_d), ("e", section_e)):
        if letter in which:
            t0 = time.time()
            run()
            out["seconds:" + letter] = time.time() - t0
            print("[grid] section %s: %.1f s" % (letter, out["seconds:" + letter]), flush=True)
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "abcde")
