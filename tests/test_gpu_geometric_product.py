"""The geometric stiffness on the device (femshell_geometric_product, FemShell.geometric_product) against
tests/helpers/buckling.py, the reference tests/test_buckling_cpu.py pins."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import buckling as bk, prescribed as pr, resultants as rs
from tests.helpers.product import ROOT, ensure_built

pytestmark = pytest.mark.gpu

pkg = ensure_built()

COLS = (1, 4, 5, 9)  # a narrow pass, a full pass, a pass plus a tail of one, two passes plus one


def _context(xyz, tri, quad, sec=None):
    fs = pkg.FemShell(rs.NU, rs.E, rs.T)
    fs.set_mesh(xyz, tri, quad)
    if sec is not None:
        fs.set_sections(sec[0], sec[1], sec[2])
    return fs


def _mask(n):
    mask = np.zeros(n, np.uint8)
    mask[::3] = 0x15
    mask[0] = 0x3F
    return mask


# ------------------------------------------------------------------ 1. device against reference

@pytest.mark.parametrize("name", list(rs.device_meshes()))
def test_product_matches_the_reference(name, monkeypatch):
    """Seeded random u and X: |Y - Y_ref| <= 1e-12 T_a per row, translation and column, for 1, 4, 5 and 9 columns.  The rotational
    rows are exactly zero, column j is bitwise the single-column call, two calls give the same bits, a Dirichlet set does not
    show."""
    xyz, tri, quad, sec, env = rs.device_meshes()[name]()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n = len(xyz)
    fs = _context(xyz, tri, quad, sec)
    u = rs.random_u(n)
    X = np.random.default_rng(31).uniform(-1.0, 1.0, (max(COLS), n, 6))
    Y_ref, Ta = bk.product(n, bk.element_coefficients(xyz, tri, quad, u, rs.NU, rs.E, rs.T, sec), X)
    worst, Y9 = 0.0, None
    for c in COLS:
        Y = fs.geometric_product(u, X[:c])
        assert Y.shape == (c, n, 6)
        ratio = bk.bound_ratio(Y, Y_ref[:c], Ta[:c])
        worst = max(worst, ratio)
        assert ratio <= 1.0, (c, ratio)
        assert np.abs(Y[:, :, :3]).max() > 0.0 and not Y[:, :, 3:].any()
        Y9 = Y
    ne = (0 if tri is None else len(tri)) + (0 if quad is None else len(quad))
    print("geometric_product_vs_reference %-28s elements %5d  max |Y - Y_ref| / (1e-12 T_a) = %.3e" % (name, ne, worst))
    for j in (0, 3, 4, 8):  # first pass, its last column, second pass, the tail
        np.testing.assert_array_equal(fs.geometric_product(u, X[j]), Y9[j], err_msg="column %d" % j)
    np.testing.assert_array_equal(fs.geometric_product(u, X), Y9)
    fs.set_dirichlet(_mask(n))
    np.testing.assert_array_equal(fs.geometric_product(u, X), Y9)
    fs.close()


def test_null_form_after_a_solve_gives_the_bits_of_the_explicit_one():
    """u None: the last solution with its prescribed part, where it lies in HBM"""
    xyz, tri = pr.panel(lift=True)
    n = len(xyz)
    mask = np.zeros(n, np.uint8)
    mask[pr.edge_nodes(xyz, 0, 0.0)] = 0x3F
    tip = pr.edge_nodes(xyz, 0, pr.LX)
    mask[tip] |= 0x01
    ubar = np.zeros((n, 6))
    ubar[tip, 0] = -1e-3
    X = np.random.default_rng(5).uniform(-1.0, 1.0, (5, n, 6))
    fs = _context(xyz, tri, None)
    fs.set_dirichlet(mask)
    fs.set_prescribed(ubar)
    fs.set_loads(np.random.default_rng(6).uniform(-1.0, 1.0, (n, 6)))
    with pytest.raises(pkg.FemShellError) as info:  # before any solve
        fs.geometric_product(None, X)
    assert info.value.code == -1
    fs.set_preconditioner("jacobi")
    u, sinfo = fs.solve(rtol=1e-12, max_it=50000)
    assert sinfo["converged"] == 1 and np.array_equal(u[tip, 0], np.full(len(tip), -1e-3))
    Y = fs.geometric_product(None, X)
    assert np.abs(Y).max() > 0.0
    np.testing.assert_array_equal(Y, fs.geometric_product(u, X))
    np.testing.assert_array_equal(fs.get_solution(), u)
    fs.close()


def test_refusals_leave_the_context_usable():
    xyz, tri = pr.panel(lift=True)
    n = len(xyz)
    u = rs.random_u(n)
    X = np.random.default_rng(5).uniform(-1.0, 1.0, (2, n, 6))
    fs = pkg.FemShell(rs.NU, rs.E, rs.T)
    dp = lambda a: a.ctypes.data_as(fs._L.femshell_geometric_product.argtypes[1])  # noqa: E731
    Y = np.zeros_like(X)
    assert fs._L.femshell_geometric_product(fs._h, dp(u), 2, dp(X), dp(Y)) == -1  # no mesh
    assert b"no mesh" in fs._L.femshell_last_error()
    fs.set_mesh(xyz, tri)
    for cols in (0, 97):
        assert fs._L.femshell_geometric_product(fs._h, dp(u), cols, dp(X), dp(Y)) == -1
        assert b"n_cols" in fs._L.femshell_last_error()
    bad = u.copy()
    bad[3, 1] = np.nan
    with pytest.raises(pkg.FemShellError) as info:
        fs.geometric_product(bad, X)
    assert info.value.code == -1 and "non-finite" in str(info.value)
    with pytest.raises(ValueError):
        fs.geometric_product(u, X[:, :-1])
    fs.set_density(7.8e-3)
    fs.set_dirichlet(_mask(n))
    fs.dynamics_begin(1e-3)
    with pytest.raises(pkg.FemShellError) as info:
        fs.geometric_product(u, X)
    assert info.value.code == -1 and "dynamics" in str(info.value)
    fs.dynamics_end()
    Y = fs.geometric_product(u, X)
    Y_ref, Ta = bk.product(n, bk.element_coefficients(xyz, tri, None, u, rs.NU, rs.E, rs.T), X)
    assert bk.bound_ratio(Y, Y_ref, Ta) <= 1.0
    fs.close()


def test_a_degenerate_element_is_reported():
    xyz = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0]], dtype=np.float64)
    tri = np.array([[0, 1, 3], [0, 1, 2]], np.int32)  # the second has no area
    fs = _context(xyz, tri, None)
    with pytest.raises(pkg.FemShellError) as info:
        fs.geometric_product(rs.random_u(4), np.ones((1, 4, 6)))
    assert info.value.code != 0 and "degenerate" in str(info.value).lower()
    fs.close()


# ------------------------------------------------------------------ 2. the timing hook

@pytest.mark.parametrize("name", ["lifted_panel", "mixed_petals24"])
def test_time_kernel_reports_the_bytes_of_the_model(name):
    """one pass of four columns: per listed entry 16 + 4 + 48 (80 with quadrilaterals) bytes, per owned row and column 24 + 48"""
    from tests.helpers import element_loads as el
    xyz, tri, quad, sec, env = rs.device_meshes()[name]()
    assert not env
    fs = _context(xyz, tri, quad)
    ms, by = fs.time_kernel(pkg.KERNEL_GEOMETRIC_PRODUCT, reps=3)  # a mesh is all it needs
    n = len(xyz)
    coeff = 80.0 if quad is not None and len(quad) else 48.0
    assert ms > 0.0 and by == (16.0 + 4.0 + coeff) * el.listed_elements(n, tri, quad) + 72.0 * n * 4
    fs.close()


# ------------------------------------------------------------------ 3. slice walk (child processes)

WORKER = os.path.join(ROOT, "tests", "helpers", "buckling_worker.py")
CHILD_TIMEOUT = 240


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """One child per grid setting, one after another; the first child that does not exit 0 ends the module (nothing more is
    started on the GPU behind a child that failed)."""
    tmp = tmp_path_factory.mktemp("geometric_product")
    got = {}
    for grid in ("default", "8", "24"):
        env = dict(os.environ)
        env.pop("FEMSHELL_SLICE_GRID", None)
        if grid != "default":
            env["FEMSHELL_SLICE_GRID"] = grid
        out = str(tmp / ("out_%s.npz" % grid))
        r = subprocess.run([sys.executable, WORKER, out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=CHILD_TIMEOUT)
        assert r.returncode == 0, "grid %s failed:\n%s" % (grid, r.stdout.decode(errors="replace")[-1500:])
        got[grid] = dict(np.load(out))
    return got


def test_more_slices_than_workgroups_give_the_bits_of_the_default_grid(runs):
    from tests.helpers.buckling_worker import problem
    xyz, tri, u, X = problem()
    n = len(xyz)
    base = runs["default"]
    assert int(base["slices"]) == 40 and base["Y"].shape == (5, n, 6) and int(base["same"]) == 1
    Y_ref, Ta = bk.product(n, bk.element_coefficients(xyz, tri, None, u, rs.NU, rs.E, rs.T), X)
    ratio = bk.bound_ratio(base["Y"], Y_ref, Ta)
    print("geometric_product_vs_reference %-28s elements %5d  max |Y - Y_ref| / (1e-12 T_a) = %.3e" % ("panel_40x30", len(tri), ratio))
    assert ratio <= 1.0
    for grid in ("8", "24"):
        run = runs[grid]
        assert (int(run["slices"]) + 7) // 8 > int(grid) // 8  # a workgroup took a second slice
        assert int(run["same"]) == 1
        np.testing.assert_array_equal(run["Y"], base["Y"], err_msg="grid " + grid)
