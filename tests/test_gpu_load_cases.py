"""Load cases on the device (femshell_solve_cases; csrc/cases.cpp, cases.hip, api_cases.cpp): a case is bit for bit what it is when
solved alone, the solutions are held to a dense long-double solve of the exported K beside femshell_solve's own error, the context
is left as it was, multigrid contexts run the cases one after another, every refusal by status and message, and the slice walk
with more slices than workgroups in processes of their own.  The restatement the iterates are compared with is
tests/helpers/load_cases.py, which tests/test_load_cases_cpu.py pins."""
import contextlib
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import elastic_support as es, load_cases as lc, resultants as rs
from tests.helpers.product import ROOT, ensure_built

pytestmark = pytest.mark.gpu

pkg = ensure_built()

MESHES = ["strip33", "coil300", "delaunay600_rcm", "mixed_petals24", "panel_three_sections", "lifted_panel_full_storage"]
EPS = np.finfo(np.float64).eps
LD = lc.LD
INVALID, UNSUPPORTED = -1, -7
N_ALL = 7
RTOL, MAX_IT = 1e-12, 20000

_contexts = {}


@contextlib.contextmanager
def environment(env):
    """the variables a mesh's context is made under (read at creation and by set_mesh), put back afterwards"""
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def coarsest_nodes(name):
    """the multigrid option of a mesh: 40, so that the small meshes get a hierarchy -- but the coil: all of its 300 triangles meet
    in one hub node, whose aggregate is seen by more fine rows than the setup packs (255: it refuses with FEMSHELL_ERR_UNSUPPORTED),
    so its multigrid context keeps one level, the dense coarsest solve"""
    return 400 if name.startswith("coil") else 40


def context(name, pc="jacobi", supports=False):
    """one context per (mesh, preconditioner, supports) for the module: (fs, mask, loads (7, n, 6))"""
    key = (name, pc, supports)
    if key not in _contexts:
        xyz, tri, quad, sec, env = rs.device_meshes()[name]()
        with environment(env):
            fs = pkg.FemShell(rs.NU, rs.E, rs.T)
            fs.set_mesh(xyz, tri, quad)
        if sec is not None:
            fs.set_sections(sec[0], sec[1], sec[2])
        if pc == "amg":
            fs.set_preconditioner("amg", coarsest_nodes=coarsest_nodes(name))
        mask = lc.mask_for(name, len(xyz))
        fs.set_dirichlet(mask)
        if supports:
            nt, nq = (0 if tri is None else len(tri)), (0 if quad is None else len(quad))
            tk, qk = es.random_moduli(nt, nq, seed=5)
            fs.set_foundation(tk, qk)
            fs.set_springs(*es.nodes_of(es.random_springs(len(xyz), seed=6)))
        _contexts[key] = (fs, mask, lc.case_loads(len(xyz), mask, N_ALL))
    return _contexts[key]


_alone = {}


def alone(name, rtol, max_it):
    """every case of the mesh solved in a call of its own: [(u (n, 6), case dict)]"""
    key = (name, rtol, max_it)
    if key not in _alone:
        fs, _, L = context(name)
        out = []
        for j in range(N_ALL):
            u, cases, info = fs.solve_cases(L[j], rtol=rtol, max_it=max_it)
            assert info["passes"] == 1 and len(cases) == 1
            out.append((u[0], cases[0]))
        _alone[key] = out
    return _alone[key]


def rel(a, b):
    a, b = np.asarray(a, dtype=LD).ravel(), np.asarray(b, dtype=LD).ravel()
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


_truth = {}


def truth(name, supports=False):
    """the exported K of the context, dense, the device's own D^-1 as an operator in long double, the masked loads and the dense
    long-double solutions of all cases"""
    key = (name, supports)
    if key not in _truth:
        fs, mask, L = context(name, supports=supports)
        fs.assemble()
        rowptr, colidx, vals, _ = fs.export_bsr()
        K = lc.dense_from_bsr(rowptr, colidx, vals)
        assert K.shape[0] <= 3600
        B = np.where(lc.free_dofs(mask), L.reshape(N_ALL, -1), 0.0)
        inv = fs.block_jacobi_export().astype(LD)
        n = len(mask)

        def Minv(r):
            return np.einsum("aij,aj->ai", inv, np.asarray(r, dtype=LD).reshape(n, 6)).reshape(-1)

        _truth[key] = (K, Minv, B, lc.dense_solve(K, B))
    return _truth[key]


# ------------------------------------------------------------------ 1. independence

@pytest.mark.parametrize("name", MESHES)
def test_a_case_is_bitwise_what_it_is_alone(name):
    """n_cases in {1, 2, 3, 4, 5, 7}, the cases in their order and in another: u and the iteration count of every case are those of
    the case solved in a call of its own -- first in a pass, in any other position, in the tail pass -- to convergence and after
    exactly 1, 2 and 5 iterations (rtol = 0), where a column that stopped early has nothing to hide behind.  Two columns of one
    pass stop at different iterations (a condition on the inputs, asserted); the zero case costs nothing; two calls agree."""
    fs, _, L = context(name)
    for rtol, max_it in ((RTOL, MAX_IT), (0.0, 1), (0.0, 2), (0.0, 5)):
        ref = alone(name, rtol, max_it)
        for order in ([0], [0, 1], [1, 0, 3], [0, 1, 2, 3], [3, 2, 1, 0], [0, 1, 2, 3, 4], [4, 0, 1, 2, 3], [0, 1, 2, 3, 4, 5, 6],
                      [6, 5, 4, 3, 2, 1, 0]):
            u, cases, info = fs.solve_cases(L[order], rtol=rtol, max_it=max_it)
            assert info["passes"] == (len(order) + 3) // 4 and info["pc_type"] == 0
            assert info["fused_product"] == (0 if name.endswith("full_storage") else 1)
            for k, j in enumerate(order):
                assert np.array_equal(u[k], ref[j][0]), (rtol, max_it, order, k)
                assert cases[k] == ref[j][1], (rtol, max_it, order, k, cases[k], ref[j][1])
            if rtol == 0.0:
                for k, j in enumerate(order):
                    want = (0, 1) if j == 2 else (max_it, 0)
                    assert (cases[k]["iterations"], cases[k]["converged"]) == want
        if rtol > 0.0:
            its = [ref[j][1]["iterations"] for j in range(N_ALL)]
            print("load_cases_iterations %-28s %s" % (name, its))
            assert all(c[1]["converged"] == 1 for c in ref) and its[2] == 0 and not ref[2][0].any()
            assert its[0] != its[1] and its[1] > 0  # two columns of the pass [0, 1, 2, 3] finish at different iterations
            again = fs.solve_cases(L, rtol=rtol, max_it=max_it)
            for j in range(N_ALL):
                assert np.array_equal(again[0][j], ref[j][0]) and again[1][j] == ref[j][1]


# ------------------------------------------------------------------ 2. scaling

@pytest.mark.parametrize("name", MESHES)
def test_a_case_scaled_by_a_power_of_two_scales_bit_for_bit(name):
    fs, _, L = context(name)
    u, cases, _ = fs.solve_cases(np.stack([L[0], 1024.0 * L[0], L[1], L[1] / 1024.0]), rtol=RTOL, max_it=MAX_IT)
    assert np.array_equal(1024.0 * u[0], u[1]) and cases[0]["iterations"] == cases[1]["iterations"] > 0
    assert np.array_equal(u[2] / 1024.0, u[3]) and cases[2]["iterations"] == cases[3]["iterations"] > 0
    assert cases[0]["rel_residual"] == cases[1]["rel_residual"]


# ------------------------------------------------------------------ 3. against the truth

def _held_to_the_truth(name, supports=False):
    """per case: error of solve_cases <= max(4 x the error of femshell_solve for the same load on the same context, 16 eps) relative
    to ||u||, iterations within +-3 (of a solve that needs no more iterations than it has unknowns: load_cases.mask_for) -- the
    project's bars for partial sums grouped differently (test_gpu_slice_walk.py,
    test_gpu_element_truth.py); the same for the iterates after exactly 1, 2 and 5 iterations against the long-double restatement
    of the lockstep recurrence with the device's own D^-1.  Returns the worst ratio error / bar."""
    fs, mask, L = context(name, supports=supports)
    K, Minv, B, U = truth(name, supports)
    worst = 0.0
    u, cases, _ = fs.solve_cases(L, rtol=RTOL, max_it=MAX_IT)
    for j in range(N_ALL):
        fs.set_loads(L[j])
        us, info = fs.solve(rtol=RTOL, max_it=MAX_IT)
        if j == 2:
            assert not u[j].any() and not us.any()
            continue
        assert cases[j]["converged"] == 1 and info["converged"] == 1
        assert info["iterations"] <= int(lc.free_dofs(mask).sum())  # a condition on the inputs: load_cases.mask_for
        assert abs(cases[j]["iterations"] - info["iterations"]) <= 3, (j, cases[j], info["iterations"])
        e_cases, e_solve = rel(u[j], U[j]), rel(us, U[j])
        bar = max(4.0 * e_solve, 16.0 * EPS)
        worst = max(worst, e_cases / bar)
        assert e_cases <= bar, (name, j, e_cases, e_solve)
    for k in (1, 2, 5):
        Xk, cols, _ = lc.lockstep(K, Minv, B, 0.0, k)
        uk, ck, _ = fs.solve_cases(L, rtol=0.0, max_it=k)
        for j in range(N_ALL):
            if j == 2:
                continue
            fs.set_loads(L[j])
            us, info = fs.solve(rtol=0.0, max_it=k)
            assert ck[j]["iterations"] == info["iterations"] == cols[j].iters == k
            e_cases, e_solve = rel(uk[j], Xk[j]), rel(us, Xk[j])
            bar = max(4.0 * e_solve, 16.0 * EPS)
            worst = max(worst, e_cases / bar)
            assert e_cases <= bar, (name, "iterate", k, j, e_cases, e_solve)
            rr = float(np.sqrt(cols[j].rr / cols[j].bb))
            assert abs(ck[j]["rel_residual"] - rr) <= 1e-10 * rr
    return worst


@pytest.mark.parametrize("name", MESHES)
def test_cases_against_the_dense_solve_and_the_restatement(name):
    worst = _held_to_the_truth(name)
    print("load_cases_vs_truth %-28s worst error / max(4 x femshell_solve's, 16 eps) = %.3f" % (name, worst))


# ------------------------------------------------------------------ 4. the context is as it was

@pytest.mark.parametrize("name", ["coil300", "lifted_panel_full_storage"])
@pytest.mark.parametrize("pc", ["jacobi", "amg"])
def test_the_context_is_as_it_was(name, pc):
    """F, the last solution, its history and a pending initial guess are the same before and after a call, and a femshell_solve
    behind the call rebuilds nothing and gives the bits it gives on a twin context that never saw the call"""
    xyz, tri, quad, sec, env = rs.device_meshes()[name]()
    twins = []
    with environment(env):
        for _ in range(2):
            fs = pkg.FemShell(rs.NU, rs.E, rs.T)
            fs.set_mesh(xyz, tri, quad)
            twins.append(fs)
    mask = lc.mask_for(name, len(xyz))
    L = lc.case_loads(len(xyz), mask, 5)
    guess = np.random.default_rng(3).uniform(-1e-3, 1e-3, (len(xyz), 6))
    results = []
    for which, fs in enumerate(twins):
        if pc == "amg":
            fs.set_preconditioner("amg", coarsest_nodes=coarsest_nodes(name))
        fs.set_dirichlet(mask)
        fs.set_loads(L[0])
        u0, info0 = fs.solve(rtol=1e-10, max_it=MAX_IT)
        hist0, F0 = fs.residual_history(), fs.export_bsr()[3]
        fs.set_initial_guess(guess)
        if which == 0:
            u, cases, info = fs.solve_cases(L[1:], rtol=1e-10, max_it=MAX_IT)
            assert all(c["converged"] == 1 for c in cases) and info["pc_type"] == (1 if pc == "amg" else 0)
            assert np.array_equal(fs.get_solution(), u0) and np.array_equal(fs.residual_history(), hist0)
            assert np.array_equal(fs.export_bsr()[3], F0)
        u1, info1 = fs.solve(rtol=1e-10, max_it=MAX_IT)  # from the pending guess
        assert info1["assemble_seconds"] == 0.0 and info1["setup_seconds"] == 0.0 and info1["pc_setup_seconds"] == 0.0
        u2, info2 = fs.solve(rtol=1e-10, max_it=MAX_IT)  # from zero again
        results.append((u0, hist0, u1, info1["iterations"], fs.residual_history(), u2, info2["iterations"]))
    for a, b in zip(*results):
        assert np.array_equal(a, b)
    assert results[0][3] != results[0][6] or not np.array_equal(results[0][2], results[0][5])  # the guess was used
    for fs in twins:
        fs.close()


@pytest.mark.parametrize("name", ["panel_three_sections", "mixed_petals24"])
def test_cases_see_the_supported_and_sectioned_matrix(name):
    """with elastic supports set (and sections, on the panel): the dense solve of the exported K + mask(K_sup)"""
    fs, _, L = context(name, supports=True)
    plain = context(name)[0].solve_cases(L[0], rtol=RTOL, max_it=MAX_IT)[0]
    worst = _held_to_the_truth(name, supports=True)
    assert rel(fs.solve_cases(L[0], rtol=RTOL, max_it=MAX_IT)[0], plain) > 1e-6  # the supports carry load
    print("load_cases_vs_truth %-28s with supports: worst error / bar = %.3f" % (name, worst))


# ------------------------------------------------------------------ 5. multigrid contexts

@pytest.mark.parametrize("name", ["coil300", "delaunay600_rcm"])
def test_multigrid_contexts_run_the_cases_one_after_another(name):
    """every case equals set_loads + solve of that case to 1e-10 relative (the solver-term bar of test_gpu_parity.py), no fused
    product, one pass per case, and the hierarchy is built once"""
    fs, _, L = context(name, pc="amg")
    u, cases, info = fs.solve_cases(L[:5], rtol=RTOL, max_it=500)
    assert info["fused_product"] == 0 and info["passes"] == 5 and info["pc_type"] == 1
    stats = fs.amg_setup_stats()
    u_again, cases_again, _ = fs.solve_cases(L[:5], rtol=RTOL, max_it=500)
    assert fs.amg_setup_stats() == stats
    for j in range(5):
        assert np.array_equal(u[j], u_again[j]) and cases[j] == cases_again[j]
        if j == 2:
            assert not u[j].any() and cases[j]["iterations"] == 0 and cases[j]["converged"] == 1
            continue
        fs.set_loads(L[j])
        us, infos = fs.solve(rtol=RTOL, max_it=500)
        assert cases[j]["converged"] == 1 and infos["converged"] == 1 and infos["pc_setup_seconds"] == 0.0
        assert rel(u[j], us) <= 1e-10, (j, rel(u[j], us))
    assert fs.amg_setup_stats() == stats


# ------------------------------------------------------------------ 6. refusals

def _raw(fs, n_cases, loads, u, rtol=1e-10, max_it=100, null_loads=False, null_u=False):
    dp = ctypes.POINTER(ctypes.c_double)
    return fs._L.femshell_solve_cases(fs._h, n_cases, None if null_loads else loads.ctypes.data_as(dp), rtol, max_it,
                                      None if null_u else u.ctypes.data_as(dp), None, None)


def _message():
    return pkg.load_library().femshell_last_error().decode()


def test_refusals_leave_a_usable_context():
    xyz, tri = rs.device_meshes()["strip33"]()[:2]
    n = len(xyz)
    mask = lc.mask_of(n)
    L = lc.case_loads(n, mask, 5)
    marker = np.full((5, n, 6), 7.25)

    def refused(fs, code, word, n_cases=5, loads=L, **kw):
        u = marker.copy()
        assert _raw(fs, n_cases, loads, u, **kw) == code, _message()
        assert word in _message(), _message()
        assert np.array_equal(u, marker)  # u_out is not written

    fs = pkg.FemShell(rs.NU, rs.E, rs.T)
    refused(fs, INVALID, "no mesh")
    fs.set_mesh(xyz, tri)
    fs.set_dirichlet(mask)
    refused(fs, INVALID, "null", null_loads=True)
    refused(fs, INVALID, "null", null_u=True)
    assert fs._L.femshell_solve_cases(None, 1, None, 1e-10, 10, None, None, None) == INVALID
    refused(fs, INVALID, "1 .. 32", n_cases=0)
    refused(fs, INVALID, "1 .. 32", n_cases=33, loads=np.zeros((33, n, 6)))
    refused(fs, INVALID, "max_it", max_it=-1)
    for bad in (np.nan, np.inf):
        Lb = L.copy()
        Lb[2, n // 2, 4] = bad  # case 3 of 5
        refused(fs, INVALID, "case 3", loads=Lb)
    fs.set_prescribed(np.full((n, 6), 1e-3))
    refused(fs, INVALID, "femshell_set_prescribed with n = 0")
    fs.set_prescribed(None)
    fs.set_density(7.8e-3)
    fs.set_loads(L[0])
    fs.dynamics_begin(1e-3)
    refused(fs, INVALID, "dynamics")
    fs.dynamics_end()
    # usable afterwards: the cases solve, and as on a context that was never refused
    u, cases, _ = fs.solve_cases(L, rtol=1e-10, max_it=MAX_IT)
    fresh = pkg.FemShell(rs.NU, rs.E, rs.T)
    fresh.set_mesh(xyz, tri)
    fresh.set_dirichlet(mask)
    uf, cf, _ = fresh.solve_cases(L, rtol=1e-10, max_it=MAX_IT)
    assert np.array_equal(u, uf) and cases == cf and all(c["converged"] == 1 for c in cases)
    with pytest.raises(ValueError):
        fs.solve_cases(np.zeros(6 * n + 1))
    fs.close()
    fresh.close()


def test_a_row_partitioned_context_is_unsupported():
    """world_size 2 without a communicator: refused before anything is touched"""
    fs = pkg.FemShell(rs.NU, rs.E, rs.T, rank=0, world_size=2)
    u = np.zeros((1, 4, 6))
    assert _raw(fs, 1, np.zeros((1, 4, 6)), u) == UNSUPPORTED and "single-rank" in _message()
    fs.close()


# ------------------------------------------------------------------ 7. more slices than workgroups

def test_more_slices_than_workgroups(tmp_path):
    """tests/helpers/load_cases_worker.py in one child per setting of FEMSHELL_SLICE_GRID (read once per process), default and 8, one
    after another; the first child that does not exit 0 ends the module.  Independence holds inside each child (asserted there);
    across the settings the partial sums are grouped differently: u to 1e-10, iterations to +-3."""
    outs = []
    for grid in (None, "8"):
        env = {k: v for k, v in os.environ.items() if k != "FEMSHELL_SLICE_GRID"}
        if grid is not None:
            env["FEMSHELL_SLICE_GRID"] = grid
        out = str(tmp_path / ("grid_%s.npz" % (grid or "default")))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "load_cases_worker.py"), out], env=env, cwd=ROOT,
                           capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            pytest.exit("load_cases_worker.py (FEMSHELL_SLICE_GRID=%s) exited with %d:\n%s\n%s" % (grid, r.returncode, r.stdout[-2000:], r.stderr[-4000:]),
                        returncode=1)
        outs.append(np.load(out))
    a, b = outs
    for name in ("delaunay600_rcm", "coil300"):
        assert int(b["walks_" + name]) > 1 and int(a["grid_" + name]) > int(b["grid_" + name]) == 8
        for j in range(N_ALL):
            ua, ub = a["u_" + name][j], b["u_" + name][j]
            if j == 2:
                assert not ua.any() and not ub.any()
                continue
            assert rel(ua, ub) <= 1e-10, (name, j, rel(ua, ub))
            assert abs(int(a["it_" + name][j]) - int(b["it_" + name][j])) <= 3
